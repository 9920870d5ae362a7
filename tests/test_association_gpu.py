"""Lab association on the MI355X (libmmgnn_assoc.so through mmgnn/assoc_ops.py): the moment planes EQUAL the loop
reference (tests/assoc_ref.py) on lattice inputs and sit inside the derived bound on generic ones, at every tile and slab
boundary of mmg_assoc_plan; exact symmetry; bitwise repeatability, eager against a replayed hipGraph; the finish EQUALS
the numpy restatement on the device's own moments and has pandas' NaN pattern; the column statistics; every refusal
before anything is enqueued; lab_association and error_association end to end, device against the numpy path."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib
from mmgnn import assoc_ops as ao
from mmgnn import association as asc
from mmgnn.model import build_model
from mmgnn.synth import make_graph
from mmgnn.train import EdgeMasker
import assoc_ref as ref
from gram_shapes import DEV, F32, PAD, dv, padded
import gram_shapes

pytestmark = pytest.mark.gpu


def row_counts(L):
    return gram_shapes.row_counts(ao.assoc_plan, ao.AS_CHUNK, L)


def shapes():
    """L: one tile (1, 3, 16), a ragged tile (17, 50), a full block (64), a diagonal and an off-diagonal block pair (65),
    three blocks (130).  The widest tables take the n that reach a new path; the narrow ones take every n."""
    out = []
    for L in (1, 3, 16, 17, 50, 64, 65, 130):
        ns = row_counts(L)
        if L in (64, 65):
            ns = [ns[2], ns[4], ns[5]]
        elif L == 130:
            ns = [ns[0], ns[4], ns[5]]
        out += [(L, n) for n in ns]
    return out


SHAPES = shapes()


@functools.lru_cache(maxsize=None)
def case(L, n, lattice):
    """-> (X host [n, L], the padded device buffer's [:, :L] view, center host, reference planes, absolute sums).  The
    padding columns hold NaN and 1e30: poison that must never be read."""
    X = ref.make_matrix(n, L, seed=L * 1000 + n, density=0.6, lattice=lattice)
    if lattice:
        center = ref.lattice_center(L, L + n)
    else:
        center = asc.host_colstats(X)[1]
    want, ab = ref.moments(X, center)
    return X, padded(X), center, want, ab


# ---------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("L, n", SHAPES)
def test_lattice_moments_equal_the_loop_reference(L, n):
    X, Xd, center, want, _ = case(L, n, True)
    assert Xd.stride(0) == L + PAD
    got = ao.assoc_moments(Xd, dv(center)).cpu().numpy()
    for k, name in enumerate(("N", "SX", "SXX", "SXY")):
        assert np.array_equal(got[k], want[k]), (name, float(np.abs(got[k] - want[k]).max()))


@pytest.mark.parametrize("L, n", SHAPES)
def test_generic_moments_are_inside_the_bound_symmetric_and_repeatable(L, n):
    X, Xd, center, want, ab = case(L, n, False)
    cd = dv(center)
    a = ao.assoc_moments(Xd, cd)
    b = ao.assoc_moments(Xd, cd)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "two runs differ"
    got = a.cpu().numpy()
    assert np.array_equal(got[0], want[0]), "counts"
    bound = ref.moment_bound(ab)
    err = np.abs(got - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"L {L} n {n}: largest |moment - fsum| / bound {worst:.3f}")
    assert np.all(err <= bound), worst
    for k in (0, 3):
        assert torch.equal(a[k].view(torch.int64), a[k].t().contiguous().view(torch.int64)), "not exactly symmetric"


def test_a_replayed_capture_is_bitwise_the_eager_call():
    """colstats, moments and finish in ONE captured hipGraph (no allocation, no memset node, no host synchronisation
    inside), one replay."""
    L, n = 65, SHAPES[-1][1]
    X, Xd, _, _, _ = case(L, n, False)

    def run():
        count, mean, n_inf = ao.assoc_colstats(Xd)
        mom = ao.assoc_moments(Xd, mean)
        return (count, mean, n_inf, mom) + ao.assoc_finish(mom, count, n, 3)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for o in outs:
        o.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    for r, e in zip(replayed, run()):
        assert torch.equal(r.view(torch.uint8), e.view(torch.uint8)), "a replayed capture differs from the eager run"


# ---------------------------------------------------------------------------------- finish
@pytest.mark.parametrize("L, n", [s for s in SHAPES if s[0] in (17, 65, 130)])
@pytest.mark.parametrize("mp", [0, 1, 2, 30])
def test_finish_equals_the_restatement_on_the_devices_own_moments(L, n, mp):
    X, Xd, center, _, _ = case(L, n, False)
    mom = ao.assoc_moments(Xd, dv(center))
    count = dv(asc.host_colstats(X)[0])
    got = ao.assoc_finish(mom, count, n, mp)
    want = asc.host_finish(mom.cpu().numpy(), count.cpu().numpy(), n, mp)
    for g, w, name in zip(got, want, ("r", "cov", "jaccard", "lift")):
        assert np.array_equal(g.cpu().numpy(), w, equal_nan=True), name


@pytest.mark.parametrize("n, L, density, mp, seed", ref.PANDAS_SHAPES)
def test_the_nan_pattern_is_pandas(n, L, density, mp, seed):
    X = ref.pandas_case(n, L, density, seed)
    frame = pd.DataFrame(X.astype(np.float64))
    got = asc.lab_correlation(dv(X), mp)
    host = asc.lab_correlation(X, mp)
    assert np.array_equal(np.isnan(got.r.cpu().numpy()), np.isnan(frame.corr(min_periods=mp).to_numpy()))
    assert np.array_equal(np.isnan(got.cov.cpu().numpy()), np.isnan(frame.cov(min_periods=mp).to_numpy()))
    assert np.array_equal(got.n.cpu().numpy(), host.n) and np.array_equal(got.count.cpu().numpy(), host.count)
    assert np.array_equal(got.jaccard.cpu().numpy(), host.jaccard, equal_nan=True)
    assert np.array_equal(got.lift.cpu().numpy(), host.lift, equal_nan=True)
    assert float(got.mean[1]) == 0.0 and float(got.mean[2]) == 2.5          # nobody has lab 1; lab 2 is constant


# ---------------------------------------------------------------------------------- column statistics
@pytest.mark.parametrize("L, n", [s for s in SHAPES if s[0] in (1, 3, 50, 65, 130)])
def test_colstats(L, n):
    """counts and n_inf EQUAL; |mean - S / count| <= (count + 8) 2^-53 x (sum of |x|) / count, S the fsum (the slack of 8
    covers the one division).  The statistics slabs are 256 rows here: one, two, and three with a ragged last one."""
    X = ref.make_matrix(n, L, seed=L + n, density=0.6).copy()
    if n > 40:
        X[7, 0], X[11, L - 1], X[n - 1, L // 2] = np.inf, -np.inf, np.inf
    count, mean, n_inf = ao.assoc_colstats(padded(X))
    want_count, s, sa, want_inf = ref.colstats(X)
    assert np.array_equal(count.cpu().numpy(), want_count) and count.dtype == torch.int64
    assert int(n_inf.item()) == want_inf == (3 if n > 40 else 0)
    m = mean.cpu().numpy()
    have = want_count > 0
    assert np.all(m[~have] == 0.0)
    exact = s[have].astype(np.longdouble) / want_count[have]
    bound = (want_count[have] + 8) * ref.U * sa[have] / want_count[have]
    assert np.all(np.abs(m[have] - exact) <= bound)
    if want_inf:
        mom = ao.assoc_moments(dv(X), mean)
        assert bool(torch.isfinite(mom).all()), "an infinite cell must enter as missing"
        hc = asc.host_colstats(X)[0]
        assert np.array_equal(mom[0].cpu().numpy().diagonal(), hc)
        with pytest.raises(ValueError, match="3 infinite"):
            asc.lab_correlation(dv(X))
        with pytest.raises(ValueError, match="3 infinite"):
            asc.pairwise_moments(dv(X))


# ---------------------------------------------------------------------------------- refusals
def test_every_refusal_comes_before_anything_is_enqueued():
    n, L = 100, 8
    X = dv(ref.make_matrix(n, L, 0))
    lib = ao.load()
    E_ARG, E_WS = _lib.MMG_E_ARG, _lib.MMG_E_WS
    out = torch.full((4, L, L), -7.0, dtype=torch.float64, device=DEV)
    count = torch.full((L,), -7, dtype=torch.int64, device=DEV)
    mean = torch.full((L,), -7.0, dtype=torch.float64, device=DEV)
    n_inf = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    center = torch.zeros(L, dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    need_m, need_c = lib.mmg_assoc_moments_ws_bytes(n, L), lib.mmg_assoc_colstats_ws_bytes(n, L)
    assert 64 < need_m < ws.numel() and 64 < need_c < ws.numel()

    def moments(n_, L_, ld, w=ws.data_ptr(), nbytes=ws.numel()):
        return lib.mmg_assoc_moments(X.data_ptr(), n_, L_, ld, center.data_ptr(), out.data_ptr(), w, nbytes, st)

    def colstats(n_, L_, ld, w=ws.data_ptr(), nbytes=ws.numel()):
        return lib.mmg_assoc_colstats(X.data_ptr(), n_, L_, ld, count.data_ptr(), mean.data_ptr(), n_inf.data_ptr(), w,
                                      nbytes, st)

    for call in (moments, colstats):
        assert call(n, 0, L) == E_ARG and call(n, ao.AS_MAX_LABS + 1, 600) == E_ARG       # L = 0, L = 513
        assert call(n, L, L - 1) == E_ARG and b"ld_x" in _lib.load().mmg_last_error()
        assert call(0, L, L) == E_ARG and call(2 ** 31 - 1, L, L) == E_ARG
        assert call(n, L, L, ws.data_ptr(), 64) == E_WS and call(n, L, L, None, 0) == E_WS
    assert moments(n, L, L, ws.data_ptr(), need_m - 1) == E_WS
    fin = [torch.full((L, L), -7.0, dtype=torch.float64, device=DEV) for _ in range(4)]
    ptrs = [f.data_ptr() for f in fin]
    assert lib.mmg_assoc_finish(out.data_ptr(), count.data_ptr(), 0, n, 1, *ptrs, None, 0, st) == E_ARG
    assert lib.mmg_assoc_finish(out.data_ptr(), count.data_ptr(), 513, n, 1, *ptrs, None, 0, st) == E_ARG
    assert lib.mmg_assoc_finish(out.data_ptr(), count.data_ptr(), L, n, -1, *ptrs, None, 0, st) == E_ARG
    assert lib.mmg_assoc_finish(None, count.data_ptr(), L, n, 1, *ptrs, None, 0, st) == E_ARG
    torch.cuda.synchronize()
    for t in [out, count, mean, n_inf] + fin:
        assert bool((t == -7).all()), "a refused call wrote something"
    with pytest.raises(_lib.MmgError, match="device tensor"):                # never the host path for host data
        ao.assoc_colstats(torch.zeros(4, 3))
    with pytest.raises(_lib.MmgError, match="labs"):
        ao.assoc_colstats(torch.zeros(4, 513, device=DEV))
    with pytest.raises(ValueError, match="labs"):
        asc.lab_correlation(torch.zeros(4, 513, device=DEV))
    assert moments(n, L, L) == 0 and colstats(n, L, L) == 0                  # and the same calls with nothing wrong run
    torch.cuda.synchronize()
    assert not bool((out == -7).any()) and not bool((count == -7).any())


# ---------------------------------------------------------------------------------- end to end
def tolerances(X):
    """Per-cell allowance between two evaluations of r and cov of the host matrix X (the device's and the numpy path's,
    whose centres differ in the last bits).  Each moment is within (nab + 8) u of its exact value relative to its
    absolute sum (u = 2^-53).  |SXY|, |SX SY / nab| <= sqrt(SXX SYY) (Cauchy-Schwarz), so cxy carries at most
    3 (nab + 8) u sqrt(SXX SYY), vx at most 3 (nab + 8) u SXX.  cov = cxy / (nab - 1): two evaluations differ by at most
    8 (nab + 8) u sqrt(SXX SYY) / (nab - 1).  r = cxy / sqrt(vx vy) adds half the relative errors of vx and vy: with
    amp = max(SXX / vx, SYY / vy) >= sqrt(SXX SYY / (vx vy)) one evaluation is within 6 (nab + 8) u amp, two differ by
    at most 16 (nab + 8) u amp (the rest covers the divisions and the square root)."""
    mom = asc.pairwise_moments(X)
    nab, sx, sxx, _ = mom.planes
    with np.errstate(all="ignore"):
        vx, vy = sxx - sx * sx / nab, sxx.T - sx.T * sx.T / nab
        amp = np.maximum(sxx / vx, sxx.T / vy)
        tol_r = 16 * (nab + 8) * ref.U * amp
        tol_cov = 8 * (nab + 8) * ref.U * np.sqrt(sxx * sxx.T) / (nab - 1)
    return tol_r, tol_cov


def compare_tables(dev, host, X, names=None):
    (da, df), (ha, hf) = dev, host
    tol_r, tol_cov = tolerances(X)
    assert torch.is_tensor(da.r) and da.r.is_cuda and isinstance(ha.r, np.ndarray)
    assert np.array_equal(da.n.cpu().numpy(), ha.n) and np.array_equal(da.count.cpu().numpy(), ha.count)
    assert np.array_equal(da.jaccard.cpu().numpy(), ha.jaccard, equal_nan=True)
    assert np.array_equal(da.lift.cpu().numpy(), ha.lift, equal_nan=True)
    for name, tol in (("r", tol_r), ("cov", tol_cov)):
        g, w = getattr(da, name).cpu().numpy(), getattr(ha, name)
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        ok = ~np.isnan(w)
        worst = float((np.abs(g - w)[ok] / tol[ok]).max())
        print(f"{name}: device against the numpy path, largest difference / allowance {worst:.3f}")
        assert worst <= 1.0, name
    assert df["comeasurement"].equals(hf["comeasurement"])
    # the long form, row by row of the same lab pair (two nearly equal |r| may swap places between the paths)
    key = ["lab_a", "lab_b"]
    assert list(df["pairs"].columns) == list(hf["pairs"].columns) == asc.PAIR_COLUMNS
    both = df["pairs"].merge(hf["pairs"], on=key, suffixes=("", "_h"))
    assert len(both) == len(df["pairs"]) == len(hf["pairs"]) > 0
    assert (both.n == both.n_h).all() and (both.jaccard == both.jaccard_h).all() and (both.lift == both.lift_h).all()
    idx = {asc._lab_name(names, i): i for i in range(ha.n.shape[0])}
    a, b = both.lab_a.map(idx).to_numpy(), both.lab_b.map(idx).to_numpy()
    t = tol_r[a, b]
    assert (np.isnan(both.r) == np.isnan(both.r_h)).all()
    ok = ~np.isnan(both.r_h.to_numpy())
    assert (np.abs(both.r - both.r_h).to_numpy()[ok] <= t[ok]).all()
    for col in ("r_lower", "r_upper"):                       # d tanh(atanh r +- h) / dr = (1 - bound^2) / (1 - r^2)
        slope = (1 - both[col + "_h"].to_numpy() ** 2) / (1 - both.r_h.to_numpy() ** 2)
        assert (np.abs(both[col] - both[col + "_h"]).to_numpy()[ok] <= 2 * t[ok] * slope[ok] + ref.U).all(), col
    dc, hc = df["coverage"], hf["coverage"]
    assert list(dc.columns) == asc.COVERAGE_COLUMNS and dc.lab.equals(hc.lab) and dc.patients.equals(hc.patients)
    assert dc.coverage.equals(hc.coverage)
    _, _, sa, _ = ref.colstats(X)
    cnt = ha.count
    assert (np.abs(dc["mean"] - hc["mean"]).to_numpy() <= 2 * (cnt + 8) * ref.U * sa / np.maximum(cnt, 1)).all()
    std = hc["std"].to_numpy()
    ok = ~np.isnan(std) & (std > 0)
    assert (np.isnan(dc["std"].to_numpy()) == np.isnan(std)).all()
    assert (np.abs(dc["std"].to_numpy() - std)[ok] <= np.diagonal(tol_cov)[ok] / std[ok]).all()


def test_lab_association_and_error_association_end_to_end(tmp_path):
    g, gd = make_graph(1, seed=0), make_graph(1, seed=0).to(DEV)
    names = asc._graph_names(g)
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    dev = asc.lab_association(gd, output_dir=tmp_path / "dev", min_periods=30)
    host = asc.lab_association(g, output_dir=tmp_path / "host", min_periods=30)
    ei = g[asc.LAB_EDGE].edge_index
    X = asc.lab_matrix(ei[0], ei[1], g[asc.LAB_EDGE].edge_attr.reshape(-1), P, L)
    compare_tables(dev, host, X, names)
    for f in ("lab_comeasurement.csv", "lab_correlation.csv", "lab_association_pairs.csv", "lab_coverage.csv"):
        assert (tmp_path / "dev" / f).exists() and (tmp_path / "host" / f).exists()
    # the residuals of a model on the test split
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (gd.node_types, gd.edge_types), None).to(DEV)
    model._init_embeddings(gd)
    masker = EdgeMasker(gd)
    dev = asc.error_association(model, gd, masker, "test", output_dir=tmp_path / "err", min_periods=10)
    R = asc.residual_matrix(model, gd, masker, "test")
    assert R.is_cuda and R.shape == (P, L) and int(torch.isfinite(R).sum()) == int(masker.test_mask.sum())
    Rh = R.cpu().numpy()
    host = asc._tables(Rh, names, 10, None, {})
    compare_tables(dev, host, Rh, names)
    assert sorted(p.name for p in (tmp_path / "err").iterdir()) == ["error_association_pairs.csv", "error_correlation.csv"]
    assert len(pd.read_csv(tmp_path / "err" / "error_association_pairs.csv")) == len(dev[1]["pairs"])
