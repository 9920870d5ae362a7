"""Chained-equations lab imputation on the MI355X (libmmgnn_chain.so through mmgnn/chain_ops.py): the row-masked
moments EQUAL the loop reference (tests/chain_ref.py) on lattice inputs and sit inside the derived bound on generic ones,
at every tile and slab boundary of mmg_chain_plan; exact symmetry; bitwise repeatability; solve, apply, init and finish
EQUAL the numpy restatement on the device's own inputs; the whole chain against the 80-bit chain with the host path's
distance as the yardstick; transform; one captured round replayed; every refusal before anything is enqueued; the
drivers, device against the numpy path."""
import functools

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib
from mmgnn import chain_ops as co
from mmgnn import chained as ch
from mmgnn import evaluate as ev
from mmgnn.association import host_colstats
from mmgnn.chained import ChainedLabImputer
from mmgnn.model import build_model
from mmgnn.synth import make_graph
from mmgnn.train import EdgeMasker
import assoc_ref
import chain_ref as ref
from gram_shapes import DEV, F32, bits, dv, padded
import gram_shapes

pytestmark = pytest.mark.gpu
LABS = (1, 2, 3, 16, 17, 50, 64, 65, 128)


def row_counts(L):
    return gram_shapes.row_counts(co.chain_plan, co.CH_CHUNK, L)


def shapes():
    """L: one tile (1, 2, 3, 16), a ragged tile (17, 50), a full block (64), a diagonal and an off-diagonal block pair
    (65), two full blocks (128).  The widest tables take the n that reach a new path; the narrow ones take every n."""
    out = []
    for L in LABS:
        ns = row_counts(L)
        if L >= 64:
            ns = [ns[2], ns[4], ns[5]]
        out += [(L, n) for n in ns]
    return out


SHAPES = shapes()


def targets(L, n):
    """The first lab, the last lab and one lab in each 16-wide tile (the widest tables at their largest n only)."""
    t = {0, L - 1}
    if L < 64 or n == row_counts(L)[5]:
        t |= {min(16 * k + 5, L - 1) for k in range((L + 15) // 16)}
    return sorted(t)


@functools.lru_cache(maxsize=None)
def case(L, n, lattice):
    """-> (X host, its padded device view, W host fp64, W device, center host): W holds X where observed and OTHER values
    elsewhere (a chain in progress), lab 1 of a table with more than two labs is one nobody has."""
    X = ref.make_matrix(n, L, seed=L * 1000 + n, density=0.6, lattice=lattice)
    if L > 2:
        X[:, 1] = np.nan
    rng = np.random.default_rng(L + n)
    if lattice:
        center = assoc_ref.lattice_center(L, L + n)
        fill = rng.integers(-40, 41, (n, L)) / 8.0
    else:
        center = host_colstats(X)[1]
        fill = rng.standard_normal((n, L)) * 2.0 + center[None, :]
    W = np.where(np.isfinite(X), X.astype(np.float64), fill)
    if L > 2:
        W[:, 1], center[1] = 0.0, 0.0
    return X, padded(X), W, dv(W), center


@functools.lru_cache(maxsize=None)
def reference(L, n, lattice, j):
    X, _, W, _, center = case(L, n, lattice)
    return ref.moments(W, X, j, center)


def device_moments(L, n, lattice, j):
    X, Xd, W, Wd, center = case(L, n, lattice)
    n_j, s, G = co.chain_moments(Wd, Xd, j, dv(center))
    return n_j, s, G


# ---------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("L, n", SHAPES)
def test_lattice_moments_equal_the_loop_reference(L, n):
    for j in targets(L, n):
        n_j, s, G = device_moments(L, n, True, j)
        wn, ws, wG, _, _ = reference(L, n, True, j)
        assert int(n_j.item()) == wn, j
        assert np.array_equal(s.cpu().numpy(), ws), (j, "s")
        assert np.array_equal(G.cpu().numpy(), wG), (j, float(np.abs(G.cpu().numpy() - wG).max()))


@pytest.mark.parametrize("L, n", SHAPES)
def test_generic_moments_are_inside_the_bound_symmetric_and_repeatable(L, n):
    worst = 0.0
    for j in targets(L, n):
        n_j, s, G = device_moments(L, n, False, j)
        n_j2, s2, G2 = device_moments(L, n, False, j)
        assert torch.equal(bits(G), bits(G2)) and torch.equal(bits(s), bits(s2)) and torch.equal(n_j, n_j2), "two runs differ"
        wn, ws, wG, sa, Ga = reference(L, n, False, j)
        assert int(n_j.item()) == wn and n_j.dtype == torch.int64, j
        assert torch.equal(bits(G), bits(G.t())), "not exactly symmetric"
        for got, want, ab in ((s.cpu().numpy(), ws, sa), (G.cpu().numpy(), wG, Ga)):
            bound = ref.moment_bound(wn, ab)
            err = np.abs(got - want)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), (j, worst)
    print(f"L {L} n {n}: largest |moment - fsum| / bound {worst:.3f}")


# ---------------------------------------------------------------------------------- init, solve, apply, finish
@pytest.mark.parametrize("L", LABS)
def test_init_and_finish_equal_the_restatement(L):
    n = row_counts(L)[5]
    X, Xd, W, Wd, center = case(L, n, False)
    count = host_colstats(X)[0]
    got = co.chain_init(Xd, dv(center)).cpu().numpy()
    assert np.array_equal(got, ch.host_init(X, center))
    out = co.chain_finish(Wd, Xd, dv(count)).cpu().numpy()
    want = ch.host_finish(W, X, count)
    assert out.dtype == F32 and np.array_equal(out, want, equal_nan=True)
    obs = np.isfinite(X)
    assert np.array_equal(out[obs].view(np.int32), X[obs].view(np.int32)), "observed cells bit for bit"
    assert np.array_equal(np.isnan(out), ~obs & (count == 0)[None, :])


def some_targets(L):
    """First, last and middle lab, without lab 1 of a table with more than two labs (nobody has it)."""
    return [0] if L < 3 else sorted({0, L - 1, L // 2} - {1})


def solve_on_device(G, s, n_j, count, j, alpha):
    L = s.numel()
    w = torch.full((L,), -7.0, dtype=torch.float64, device=DEV)
    mu = torch.full((L,), -7.0, dtype=torch.float64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int64, device=DEV)
    co.chain_solve(G, s, n_j, count, j, alpha, w, mu, bad)
    return w.cpu().numpy(), mu.cpu().numpy(), int(bad.item())


@pytest.mark.parametrize("alpha", [1.0, 0.03])
@pytest.mark.parametrize("L", LABS)
def test_solve_equals_the_restatement_on_the_devices_own_moments(L, alpha):
    n = row_counts(L)[5]
    X, Xd, W, Wd, center = case(L, n, False)
    count = host_colstats(X)[0]
    for j in some_targets(L):
        n_j, s, G = device_moments(L, n, False, j)
        w, mu, bad = solve_on_device(G, s, n_j, dv(count), j, alpha)
        ww, wmu, wbad = ch.host_solve(G.cpu().numpy(), s.cpu().numpy(), int(n_j.item()), count, j, alpha)
        assert bad == wbad == 0
        assert np.array_equal(mu, wmu) and np.array_equal(w, ww), (j, float(np.abs(w - ww).max()))
        assert w[j] == 0.0 and (L < 3 or w[1] == 0.0) and (L < 3 or np.count_nonzero(w) == L - 2)


def test_solve_with_one_row_identical_columns_and_a_bad_pivot():
    n, L = 300, 9
    X = ref.make_matrix(n, L, seed=2, density=0.7)
    X[:, 3] = np.nan
    X[41, 3] = F32(1.75)                                   # n_j = 1
    X[:, 6] = X[:, 5]                                      # identical columns
    count, center, _ = host_colstats(X)
    Xd, cd = padded(X), dv(center)
    Wd = co.chain_init(Xd, cd)
    n_j, s, G = co.chain_moments(Wd, Xd, 3, cd)
    assert int(n_j.item()) == 1
    w, mu, bad = solve_on_device(G, s, n_j, dv(count), 3, 1.0)
    ww, wmu, _ = ch.host_solve(G.cpu().numpy(), s.cpu().numpy(), 1, count, 3, 1.0)
    assert bad == 0 and np.all(w == 0.0) and np.array_equal(mu, wmu) and np.array_equal(w, ww), "one row: C = 0, w = 0"
    for j in (5, 0):
        n_j, s, G = co.chain_moments(Wd, Xd, j, cd)
        w, mu, bad = solve_on_device(G, s, n_j, dv(count), j, 1e-6)
        ww, wmu, wbad = ch.host_solve(G.cpu().numpy(), s.cpu().numpy(), int(n_j.item()), count, j, 1e-6)
        assert bad == wbad and np.array_equal(w, ww) and np.array_equal(mu, wmu), j
    # a constructed system whose pivots are -5 + 1: the counter fires once per predictor, on the device as on the host
    G = dv(-5.0 * np.eye(L))
    s, n_j = torch.zeros(L, dtype=torch.float64, device=DEV), torch.full((1,), 10, dtype=torch.int64, device=DEV)
    _, _, bad = solve_on_device(G, s, n_j, dv(np.full(L, 10, np.int64)), 2, 1.0)
    assert bad == L - 1 == ch.host_solve(-5.0 * np.eye(L), np.zeros(L), 10, np.full(L, 10), 2, 1.0)[2]


@pytest.mark.parametrize("L", LABS)
def test_apply_equals_the_restatement(L):
    n = row_counts(L)[5]
    X, Xd, W, _, center = case(L, n, False)
    count = host_colstats(X)[0]
    rng = np.random.default_rng(L)
    lo, hi = np.full(L, -np.inf), np.full(L, np.inf)
    lo[0], hi[0] = center[0] - 0.5, center[0] + 0.25         # the first lab is clipped on both sides
    Wd, Wh = dv(W), W.copy()
    delta = torch.full((1,), 1e9, dtype=torch.float64, device=DEV)
    for k, j in enumerate(some_targets(L)):
        w = rng.standard_normal(L) / np.sqrt(L)
        mu = rng.standard_normal(L) * 0.1
        w[j] = 0.0
        co.chain_apply(Wd, Xd, j, dv(count), dv(center), dv(w), dv(mu), dv(lo), dv(hi), delta, accumulate=k > 0)
        want = ch.host_apply(Wh, X, j, count, center, w, mu, lo, hi)
        assert np.array_equal(Wd.cpu().numpy(), Wh), j
        top = want if k == 0 else max(top, want)
        assert float(delta.item()) == top, "the maximum equals numpy's (the first call overwrites, the later ones fold)"
    miss = ~np.isfinite(X[:, 0])
    got = Wd.cpu().numpy()[miss, 0]
    assert miss.sum() > 100 and np.all(got >= lo[0]) and np.all(got <= hi[0])
    assert L == 1 or ((got == lo[0]).any() and (got == hi[0]).any()), "with a predictor the clips bind on both sides"
    obs = np.isfinite(X)
    assert np.array_equal(Wd.cpu().numpy()[obs], X[obs].astype(np.float64)), "observed cells are never written"


# ---------------------------------------------------------------------------------- the whole chain
CHAIN_SHAPES = [(70, 5), (300, 17), (1000, 65), (200, 128)]


@functools.lru_cache(maxsize=None)
def chain_case(n, L):
    X = ref.make_matrix(n, L, seed=n + L, density=0.6)
    host = ChainedLabImputer(alpha=1.0, max_iter=3, tol=0).fit_matrix(X)
    want, labs, _ = ref.chain(X, 1.0, 3)
    return X, host, want, labs


@pytest.mark.parametrize("n, L", CHAIN_SHAPES)
def test_the_whole_chain_against_the_80_bit_chain(n, L):
    """Three rounds, tol = 0: the device is at most 8 x as far from the 80-bit chain as the host path is."""
    X, host, want, labs = chain_case(n, L)
    Xd = padded(X)
    imp = ChainedLabImputer(alpha=1.0, max_iter=3, tol=0).fit_matrix(Xd)
    W = imp.imputed64_.cpu().numpy()
    d_dev = float(np.abs(W.astype(ref.LD) - want).max())
    d_host = float(np.abs(host.imputed64_.astype(ref.LD) - want).max())
    print(f"({n}, {L}): device {d_dev:.2e}, host path {d_host:.2e} from the 80-bit chain")
    assert d_host > 0 and d_dev <= 8 * d_host
    assert imp.n_iter_ == host.n_iter_ == 3 and imp._state["order"].tolist() == labs == host._state["order"].tolist()
    assert np.allclose(imp.history_, host.history_, rtol=1e-9, atol=0)
    out = imp.impute_matrix()
    assert out.is_cuda and out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), W.astype(F32))
    obs = np.isfinite(X)
    assert np.array_equal(out.cpu().numpy()[obs].view(np.int32), X[obs].view(np.int32))
    # transform of the training matrix is bitwise the fit; new rows EQUAL the host path on the device's coefficients
    assert torch.equal(bits(imp.transform(Xd)), bits(out))
    Xn = ref.make_matrix(77, L, seed=9 * n + L, density=0.5)
    got = imp.transform(padded(Xn), return_float64=True).cpu().numpy()
    assert np.array_equal(got, imp.transform(Xn, return_float64=True))
    assert np.array_equal(imp.transform(padded(Xn)).cpu().numpy(), imp.transform(Xn))
    rows = torch.tensor([3, 0, n - 1], device=DEV)
    assert torch.equal(imp.impute_matrix(rows), out[rows])
    assert torch.equal(imp.predict(rows, torch.tensor([0, L - 1, L // 2], device=DEV)), out[rows, [0, L - 1, L // 2]])
    # a state loaded elsewhere transforms on the device without the training matrix
    other = ChainedLabImputer().load_state_dict(imp.state_dict())
    assert torch.equal(bits(other.transform(Xd)), bits(out))


@pytest.mark.parametrize("n, L", CHAIN_SHAPES[:2])
def test_the_stopping_rule_on_the_device(n, L):
    X = ref.make_matrix(n, L, seed=n + L, density=0.6)
    h = ChainedLabImputer(max_iter=10, tol=0).fit_matrix(X).history_
    k = max(i for i in range(1, 10) if h[i] < min(h[:i]) / 1.5)
    top = float(np.nanmax(np.abs(X)))
    tol = float(np.sqrt(h[k] * min(h[:k]))) / top
    assert min(h[:k]) > 1.2 * tol * top and h[k] < tol * top / 1.2, "an asserted gap: rounding cannot cross it"
    imp = ChainedLabImputer(max_iter=10, tol=tol).fit_matrix(padded(X))
    assert imp.n_iter_ == k + 1 and len(imp.history_) == k + 1 and np.allclose(imp.history_, h[:k + 1], rtol=1e-9, atol=0)
    assert imp._state["coef"].shape == (k + 1, L, 2, L)


def test_a_replayed_captured_round_is_bitwise_the_eager_round():
    """One round of the (300, 17) chain -- 3 calls per lab -- in ONE captured hipGraph (no allocation, no memset node, no
    host synchronisation inside), one replay."""
    n, L = 300, 17
    X = ref.make_matrix(n, L, seed=n + L, density=0.6)
    Xd = padded(X)
    count_h, center_h, _ = host_colstats(X)
    order = ch.visit_order(count_h, n)
    lo, hi = np.full(L, -np.inf), np.full(L, np.inf)

    def new_chain():
        return ch._DeviceChain(Xd, dv(count_h), dv(center_h), order, 1.0, lo, hi, 1)

    eager = new_chain()
    eager.round(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        new_chain().round(0)                                 # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    captured = new_chain()
    start = captured.W.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.round(0)
    captured.W.copy_(start)
    captured.coef.fill_(-1)
    captured.stat.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name in ("W", "coef", "stat"):
        assert torch.equal(bits(getattr(captured, name)), bits(getattr(eager, name))), name
    assert float(eager.delta(0).item()) > 0 and int(eager.stat[0, 1]) == 0


# ---------------------------------------------------------------------------------- refusals
def test_every_refusal_comes_before_anything_is_enqueued():
    n, L = 100, 8
    X = dv(ref.make_matrix(n, L, 0))
    lib = co.load()
    E_ARG, E_WS = _lib.MMG_E_ARG, _lib.MMG_E_WS
    f64 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=DEV)      # noqa: E731
    i64 = lambda *shape: torch.full(shape, -7, dtype=torch.int64, device=DEV)          # noqa: E731
    W, G, s, w, mu, delta, n_j, bad = f64(n, L), f64(L, L), f64(L), f64(L), f64(L), f64(1), i64(1), i64(1)
    out = torch.full((n, L), -7.0, dtype=torch.float32, device=DEV)
    center, count = torch.zeros(L, dtype=torch.float64, device=DEV), torch.full((L,), 5, dtype=torch.int64, device=DEV)
    lo, hi = f64(L), f64(L)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    need_m, need_a = lib.mmg_chain_moments_ws_bytes(n, L), lib.mmg_chain_apply_ws_bytes(n, L)
    assert 64 < need_m < ws.numel() and 64 < need_a < ws.numel()
    p = lambda t: t.data_ptr()                                                          # noqa: E731

    def moments(n_, L_, ld, j=0, w_=ws.data_ptr(), nbytes=ws.numel()):
        return lib.mmg_chain_moments(p(W), p(X), n_, L_, ld, j, p(center), p(n_j), p(s), p(G), w_, nbytes, st)

    def apply(n_, L_, ld, j=0, w_=ws.data_ptr(), nbytes=ws.numel()):
        return lib.mmg_chain_apply(p(W), p(X), n_, L_, ld, j, p(count), p(center), p(w), p(mu), p(lo), p(hi), 0, p(delta),
                                   w_, nbytes, st)

    for call in (moments, apply):
        assert call(n, 0, L) == E_ARG and call(n, co.CH_MAX_LABS + 1, 200) == E_ARG
        assert call(n, L, L - 1) == E_ARG and b"ld_x" in _lib.load().mmg_last_error()
        assert call(0, L, L) == E_ARG and call(2 ** 31 - 1, L, L) == E_ARG
        assert call(n, L, L, -1) == E_ARG and call(n, L, L, L) == E_ARG
        assert call(n, L, L, 0, ws.data_ptr(), 64) == E_WS and call(n, L, L, 0, None, 0) == E_WS
    assert moments(n, L, L, 0, ws.data_ptr(), need_m - 1) == E_WS
    assert lib.mmg_chain_init(p(X), n, L, L - 1, p(center), p(W), st) == E_ARG
    assert lib.mmg_chain_init(p(X), n, L, L, None, p(W), st) == E_ARG
    assert lib.mmg_chain_solve(p(G), p(s), p(n_j), p(count), L, 0, 0.0, p(w), p(mu), p(bad), st) == E_ARG
    assert lib.mmg_chain_solve(p(G), p(s), p(n_j), p(count), L, L, 1.0, p(w), p(mu), p(bad), st) == E_ARG
    assert lib.mmg_chain_solve(p(G), p(s), p(n_j), p(count), 129, 0, 1.0, p(w), p(mu), p(bad), st) == E_ARG
    assert lib.mmg_chain_solve(p(G), p(s), None, p(count), L, 0, 1.0, p(w), p(mu), p(bad), st) == E_ARG
    assert lib.mmg_chain_finish(p(W), p(X), n, L, L, p(count), p(out), L - 1, st) == E_ARG
    assert lib.mmg_chain_finish(p(W), p(X), n, L, L, None, p(out), L, st) == E_ARG
    torch.cuda.synchronize()
    for t in (W, G, s, w, mu, delta, n_j, bad, out):
        assert bool((t == -7).all()), "a refused call wrote something"
    with pytest.raises(_lib.MmgError, match="device tensor"):                # never the host path for host data
        co.chain_init(torch.zeros(4, 3), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(_lib.MmgError, match="labs"):
        co.chain_init(torch.zeros(4, 129, device=DEV), torch.zeros(129, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="labs"):
        ChainedLabImputer().fit_matrix(torch.zeros(4, 129, device=DEV))
    bad_x = X.clone()
    bad_x[3, 2] = float("inf")
    with pytest.raises(ValueError, match="1 infinite"):
        ChainedLabImputer().fit_matrix(bad_x)
    assert moments(n, L, L) == 0 and apply(n, L, L) == 0                     # and the same calls with nothing wrong run
    torch.cuda.synchronize()
    assert not bool((G == -7).any()) and not bool((delta == -7).any())


# ---------------------------------------------------------------------------------- the drivers
def ulp32(x):
    return np.abs(np.asarray(x, np.float64)) * 2.0 ** -23 + 2.0 ** -149


def test_the_drivers_device_against_the_numpy_path(tmp_path):
    """The imputed fp32 cells of the two paths are the one rounding of two fp64 chains 1e-12 apart: at most one fp32 ulp
    apart, and a mean absolute error over them moves by no more than the largest such ulp."""
    from mmgnn import bootstrap as bt
    g = make_graph(1, seed=0)
    gd = make_graph(1, seed=0).to(DEV)
    host = ev.evaluate_chained_baseline(g, EdgeMasker(g), "test", max_iter=3, tol=0.0)["chained_equations"]
    masker = EdgeMasker(gd)
    dev = ev.evaluate_chained_baseline(gd, masker, "test", max_iter=3, tol=0.0)["chained_equations"]
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    tr_ei, tr_v, _, _ = masker.get_masked_data("train", want_mask=False)
    te_ei, te_v, _, _ = masker.get_masked_data("test", want_mask=False)
    tr_ei, tr_v, te_ei = tr_ei.to(DEV), tr_v.to(DEV).reshape(-1).float(), te_ei.to(DEV)
    d_imp = ChainedLabImputer(max_iter=3, tol=0.0).fit(tr_ei[0], tr_ei[1], tr_v, P, L)
    h_imp = ChainedLabImputer(max_iter=3, tol=0.0).fit(tr_ei[0].cpu().numpy(), tr_ei[1].cpu().numpy(), tr_v.cpu().numpy(),
                                                      P, L)
    a, b = d_imp.impute_matrix().cpu().numpy(), h_imp.impute_matrix()
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(b)] <= ulp32(b)[~np.isnan(b)])
    top = float(ulp32(np.nanmax(np.abs(b))))
    print(f"synthetic x1, test split: chained_equations MAE device {dev['mae']:.6f} host {host['mae']:.6f}")
    # the driver is the imputer read at the split's pairs, through the same metric function
    y = te_v.cpu().numpy().reshape(-1)
    assert dev == ev.compute_regression_metrics(d_imp.predict(te_ei[0], te_ei[1]).cpu().numpy(), y)
    assert host == ev.compute_regression_metrics(h_imp.predict(te_ei[0].cpu().numpy(), te_ei[1].cpu().numpy()), y)
    assert set(dev) == set(host) and np.isfinite(dev["mae"])
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}, "evaluation": {"stratify_by": []}}
    torch.manual_seed(0)
    model = build_model(cfg, (gd.node_types, gd.edge_types), None).to(DEV)
    model._init_embeddings(gd)
    out = bt.evaluate_with_intervals(model, gd, masker, cfg, tmp_path, replicates=20,
                                     baselines=("per_lab_mean", "chained_equations"))
    rows = {(r["baseline"], r["metric"]): r for r in out["baseline_comparison"]}
    assert {k[0] for k in rows} == {"per_lab_mean", "chained_equations"}
    model_mae = out["overall"][0]["estimate"]
    full = ChainedLabImputer().fit(tr_ei[0].cpu().numpy(), tr_ei[1].cpu().numpy(), tr_v.cpu().numpy(), P, L)
    pred = full.predict(te_ei[0].cpu().numpy(), te_ei[1].cpu().numpy()).astype(np.float64)
    want = float(np.abs(pred - te_v.cpu().numpy().reshape(-1).astype(np.float64)).mean())
    got = model_mae - rows[("chained_equations", "mae")]["estimate"]
    assert abs(got - want) <= top + 1e-6 * want              # 1e-6: the allowance test_bootstrap_gpu gives this estimate
