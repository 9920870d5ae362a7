"""Measurement propensity on the MI355X (libmmgnn_prop.so through mmgnn/prop_ops.py): the indicator EQUAL; the link's z
EQUAL numpy and its p, q, s, r and loss against 80-bit values with the restatement's own distance as the yardstick; the
weighted moments EQUAL the exact sums on lattice inputs and inside the derived bound on generic ones, at every tile and
slab boundary of mmg_prop_plan, exactly symmetric, every cell written once, bitwise repeatable; solve and update EQUAL
the numpy restatement on the device's own H, g and state; the whole fit against the 80-bit Newton; frozen labs; one
captured round replayed; predict; the weighted error sums over pairs EQUAL the restatement in shuffled and lab-major order;
the drivers, device against the numpy path."""
import functools

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib
from mmgnn import missingness as ms
from mmgnn import prop_ops as po
from mmgnn.missingness import LabPropensity
from mmgnn.synth import make_graph
import prop_ref as ref
from gram_shapes import DEV, F32, bits, dv, padded
import gram_shapes

pytestmark = pytest.mark.gpu
FEATURES = (1, 2, 15, 16, 62, 63, 64, 127, 128)      # the table is D + 2 wide: one tile, a ragged tile, the 64 and 128 edges
HOST_DISTANCE = 1.4e-12                              # the host path's distance from the 80-bit Newton
TOL = 1e-12


def row_counts(D):
    return gram_shapes.row_counts(po.prop_plan, po.PR_CHUNK, D)


def shapes():
    out = []
    for D in FEATURES:
        ns = row_counts(D)
        if D >= 62:
            ns = [ns[2], ns[4], ns[5]]
        out += [(D, n) for n in ns]
    return out


SHAPES = shapes()
NB = 3                                               # labs of a moments case; the middle one is frozen


def f64(*shape, fill=float("nan")):
    return torch.full(shape, fill, dtype=torch.float64, device=DEV)


def state_of(active):
    st = np.zeros((len(active), po.PR_STATE), np.int32)
    st[:, po.ACTIVE] = active
    return st


# ---------------------------------------------------------------------------------- indicator, count
@pytest.mark.parametrize("n, L", [(1, 1), (300, 3), (257, 50), (70, 512)])
def test_indicator_and_count_equal_numpy(n, L):
    rng = np.random.default_rng(n + L)
    X = rng.standard_normal((n, L)).astype(F32)
    X[rng.random((n, L)) < 0.4] = np.nan
    X[rng.random((n, L)) < 0.02] = np.inf
    X[0, 0] = -np.inf
    Y, F = po.prop_indicator(padded(X), features=True)
    want = np.isfinite(X)
    assert Y.dtype == torch.uint8 and np.array_equal(Y.cpu().numpy(), want.astype(np.uint8))
    assert F.dtype == torch.float32 and np.array_equal(F.cpu().numpy(), want.astype(F32))
    assert torch.equal(po.prop_indicator(padded(X)), Y)
    count = po.prop_count(Y)
    assert count.dtype == torch.int64 and np.array_equal(count.cpu().numpy(), want.sum(0))
    wide = torch.zeros(n, L + 3, dtype=torch.uint8, device=DEV)
    wide[:, L:] = 1                                                  # padding that must not be counted
    wide[:, :L] = Y
    assert torch.equal(po.prop_count(wide[:, :L]), count)


# ---------------------------------------------------------------------------------- link
def run_link(X, mean, Y, coef, state=None, j0=0, nb=None):
    n, L = Y.shape
    nb = L if nb is None else nb
    sr, lossp, z, pq = f64(2, nb, n), f64(nb, po.link_blocks(n)), f64(nb, n), f64(2, nb, n)
    po.prop_link(padded(X), dv(mean), dv(Y), j0, nb, dv(coef), None if state is None else dv(state), sr, lossp, z=z, pq=pq)
    return [t.cpu().numpy() for t in (z, pq, sr, lossp)]


@pytest.mark.parametrize("D, n", [(1, 31), (3, 300), (17, 589), (64, 257), (128, 130)])
def test_link_z_equals_numpy_and_the_rest_meets_80_bit_values(D, n):
    rng = np.random.default_rng(D + n)
    X = rng.standard_normal((n, D)).astype(F32)
    mean = X.astype(np.float64).mean(0)
    Y = (rng.random((n, 5)) < np.array([0.5, 0.03, 0.9, 0.5, 0.5])).astype(np.uint8)
    coef = rng.standard_normal((5, D + 1)) * np.array([0.3, 1.0, 3.0, 10.0, 0.0])[:, None] / np.sqrt(D)
    z, pq, sr, lossp = run_link(X, mean, Y, coef)
    worst = {}
    for j in range(5):
        hz, hp, hq, hs, hr, ht = ms.host_link(X, mean, Y[:, j], coef[j])
        assert np.array_equal(z[j], hz), (j, "z")
        want = ref.link_from_z(hz, Y[:, j])
        for name, got, host, w in zip("pqsr", (pq[0, j], pq[1, j], sr[0, j], sr[1, j]), (hp, hq, hs, hr), want):
            yard = max(ref.rel_distance(host, w), ref.U)             # the restatement's own distance, at least one rounding
            d = ref.rel_distance(got, w)
            worst[name] = max(worst.get(name, 0.0), d / yard)
            assert d <= 8 * yard, (j, name, d, yard)
        assert np.all(np.abs((pq[0, j] + pq[1, j]) - 1.0) <= 2.0 ** -52)
        t80 = np.zeros(po.link_blocks(n) * 64, ref.LD)
        t80[:n] = want[4]
        exact, floor = t80.reshape(-1, 64).sum(1), ref.U * float(np.abs(t80).reshape(-1, 64).sum(1).max())
        yard = max(float(np.abs(ms.host_loss_blocks(ht).astype(ref.LD) - exact).max()), floor)
        d = float(np.abs(lossp[j].astype(ref.LD) - exact).max())
        worst["loss"] = max(worst.get("loss", 0.0), d / yard)
        assert lossp.shape[1] == exact.size and d <= 8 * yard, (j, "loss", d, yard)
    print(f"D {D} n {n}: largest device distance / restatement's distance from the 80-bit values {worst}")


def test_link_over_the_whole_range_of_z_and_the_stated_loss_tree():
    x = np.linspace(-745.0, 745.0, 2981).astype(F32)[:, None]
    y = (np.arange(x.size) % 2).astype(np.uint8)[:, None]
    z, pq, sr, lossp = run_link(x, np.zeros(1), y, np.array([[1.0, 0.0]]))
    assert np.array_equal(z[0], x[:, 0].astype(np.float64))
    for v in (pq, sr, lossp):
        assert np.isfinite(v).all()
    assert np.all(np.abs((pq[0, 0] + pq[1, 0]) - 1.0) <= 2.0 ** -52) and pq[0, 0, 0] < 1e-300 and pq[1, 0, -1] < 1e-300
    # the tree: lattice loss terms (z a multiple of 64, so log1p(e) = 0 or e below half an ulp) add exactly
    n = 64 * 3 + 7
    xi = (64.0 * np.random.default_rng(0).integers(1, 9, n)).astype(F32)[:, None]
    yi = np.zeros((n, 1), np.uint8)
    z, pq, sr, lossp = run_link(xi, np.zeros(1), yi, np.array([[1.0, 0.0]]))
    t = ms.host_link(xi, np.zeros(1), yi[:, 0], np.array([1.0, 0.0]))[5]
    assert np.array_equal(t, xi[:, 0].astype(np.float64)) and np.array_equal(lossp[0], ms.host_loss_blocks(t))


def test_link_leaves_a_frozen_lab_alone():
    X, y = ref.make_data("generic", 300, 3, 1)
    Y = np.stack([y, y, y], axis=1)
    z, pq, sr, lossp = run_link(X, X.astype(np.float64).mean(0), Y, np.zeros((3, 4)), state=state_of([1, 0, 1]))
    for v in (z, pq[0], pq[1], sr[0], sr[1], lossp):
        assert np.isnan(v[1]).all() and np.isfinite(v[0]).all() and np.array_equal(v[0], v[2])


# ---------------------------------------------------------------------------------- moments
@functools.lru_cache(maxsize=None)
def moment_case(D, n, lattice):
    if lattice:
        X, mean, _, _ = ref.lattice_case(n, D, D * 1000 + n)
        rng = np.random.default_rng(D + n)
        S, R = rng.integers(0, 5, (NB, n)) / 16.0, rng.integers(-16, 17, (NB, n)) / 16.0
    else:
        rng = np.random.default_rng(D * 1000 + n + 1)
        X = (rng.standard_normal((n, D)) * 2.0 + 0.5).astype(F32)
        mean = X.astype(np.float64).mean(0)
        p = rng.random((NB, n))
        S, R = p * (1 - p), p - (rng.random((NB, n)) < 0.5)
    return X, mean, S, R


def device_moments(D, n, lattice, active=(1, 0, 1)):
    X, mean, S, R = moment_case(D, n, lattice)
    H, g = f64(NB, D + 1, D + 1), f64(NB, D + 1)
    po.prop_moments(padded(X), dv(mean), dv(np.stack([S, R])), NB, 0, NB, dv(state_of(active)), H, g)
    return H, g


@pytest.mark.parametrize("D, n", SHAPES)
def test_lattice_moments_equal_the_exact_sums(D, n):
    X, mean, S, R = moment_case(D, n, True)
    H, g = device_moments(D, n, True)
    for k in (0, 2):
        wH, wg = ref.exact_moments(X, mean, S[k], R[k])
        assert np.array_equal(g[k].cpu().numpy(), wg), (k, "g")
        assert np.array_equal(H[k].cpu().numpy(), wH), (k, float(np.abs(H[k].cpu().numpy() - wH).max()))
    assert torch.isnan(H[1]).all() and torch.isnan(g[1]).all(), "a frozen lab is not written"


@pytest.mark.parametrize("D, n", SHAPES)
def test_generic_moments_are_inside_the_bound_symmetric_written_once_and_repeatable(D, n):
    X, mean, S, R = moment_case(D, n, False)
    H, g = device_moments(D, n, False, active=(1, 1, 1))
    H2, g2 = device_moments(D, n, False, active=(1, 1, 1))
    assert torch.equal(bits(H), bits(H2)) and torch.equal(bits(g), bits(g2)), "two runs differ"
    assert not torch.isnan(H).any() and not torch.isnan(g).any(), "a cell of the poisoned output was not written"
    assert torch.equal(bits(H), bits(H.transpose(1, 2))), "not exactly symmetric"
    worst = 0.0
    for k in range(NB):
        wH, wg, Ha, ga = ref.moments(X, mean, S[k], R[k])
        for got, want, ab in ((H[k].cpu().numpy(), wH, Ha), (g[k].cpu().numpy(), wg, ga)):
            bound = ref.moment_bound(n, ab)
            err = np.abs(got - want)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), (k, worst)
    print(f"D {D} n {n}: largest |moment - reference| / bound {worst:.3f}")


def test_moments_without_a_state_work_on_every_lab_and_on_a_later_batch():
    D, n = 17, 589
    X, mean, S, R = moment_case(D, n, True)
    H, g = f64(2, D + 1, D + 1), f64(2, D + 1)
    po.prop_moments(padded(X), dv(mean), dv(np.stack([S[1:], R[1:]])), 7, 5, 2, None, H, g)
    for k in range(2):
        wH, wg = ref.exact_moments(X, mean, S[1 + k], R[1 + k])
        assert np.array_equal(H[k].cpu().numpy(), wH) and np.array_equal(g[k].cpu().numpy(), wg)
    st = state_of([0, 0, 0, 0, 0, 0, 1])                              # lab j0 + 1 = 6 is the live one
    H2, g2 = f64(2, D + 1, D + 1), f64(2, D + 1)
    po.prop_moments(padded(X), dv(mean), dv(np.stack([S[1:], R[1:]])), 7, 5, 2, dv(st), H2, g2)
    assert torch.isnan(H2[0]).all() and torch.equal(bits(H2[1]), bits(H[1])) and torch.equal(bits(g2[1]), bits(g[1]))


# ---------------------------------------------------------------------------------- solve, update
class Lockstep:
    """Three labs on the device and, fed with the device's own loss sums, direction and decrement, on the host."""

    def __init__(self, D, n=589, C=1.0, tol=1e-10, max_iter=6):
        X = np.random.default_rng(D).standard_normal((n, D)).astype(F32)
        w = np.random.default_rng(D + 1).standard_normal(D) / np.sqrt(D)
        z = X.astype(np.float64) @ w
        Y = np.stack([z + np.random.default_rng(D + 2).logistic(size=n) > 0, z > 2.2, z > 0], axis=1).astype(np.uint8)
        self.X, self.Y, self.mean, self.C, self.n, self.D = X, Y, X.astype(np.float64).mean(0), C, n, D
        self.thr, self.max_iter = tol * n, max_iter
        trial, state, _ = ms.start_point(Y.sum(0), n, D)
        self.host = dict(trial=trial, beta=trial.copy(), step=np.zeros_like(trial), fstate=np.zeros((3, ms.N_FSTATE)), state=state)
        self.dev = ms._DeviceFit(padded(X), dv(self.mean), dv(Y), trial.copy(), state.copy(), C, self.thr, max_iter)

    def round(self):
        d, h = self.dev, self.host
        sr, lossp, H, g, delta, dec = d.views(3)
        active = h["state"][:, ms.ACTIVE].copy()
        po.prop_link(d.X, d.mean, d.Y, 0, 3, d.trial, d.state, sr, lossp)
        po.prop_moments(d.X, d.mean, sr, 3, 0, 3, d.state, H, g)
        delta.fill_(float("nan"))
        dec.fill_(float("nan"))
        po.prop_solve(H, g, d.trial, 0, self.C, d.state, delta, dec)
        Hh, gh, dl, dc, lp = (t.cpu().numpy() for t in (H, g, delta, dec, lossp))
        for j in range(3):
            if not active[j]:
                assert np.isnan(dl[j]).all() and np.isnan(dc[j]), "the solve of a frozen lab wrote"
                continue
            assert np.array_equal(Hh[j], Hh[j].T)
            wd, wdec, bad = ms.host_solve(Hh[j], gh[j], h["trial"][j], self.C)
            assert bad == 0 and np.array_equal(dl[j], wd) and dc[j] == wdec, (j, float(np.abs(dl[j] - wd).max()))
            ms.host_update(lp[j], dl[j], dc[j], self.C, self.thr, self.max_iter, h["beta"][j], h["trial"][j], h["step"][j],
                           h["fstate"][j], h["state"][j])
        po.prop_update(lossp, self.n, 0, delta, dec, self.C, self.thr, self.max_iter, d.beta, d.trial, d.step, d.fstate, d.state)
        for name in ("beta", "trial", "step", "fstate", "state"):
            assert np.array_equal(getattr(d, name).cpu().numpy(), h[name]), name


@pytest.mark.parametrize("D", [1, 16, 63, 64, 128])
def test_solve_and_update_equal_the_restatement_on_the_devices_own_moments(D):
    run = Lockstep(D)
    for _ in range(run.max_iter + 1):
        run.round()
    st = run.host["state"]
    assert not st[:, ms.ACTIVE].any() and st[:, ms.N_ITER].max() <= run.max_iter and st[:, ms.CONVERGED].any()
    assert len(set(st[:, ms.N_ITER].tolist())) > 1, "the labs stop in different rounds"


def test_a_pivot_that_is_not_positive_is_counted_not_hidden():
    D, L = 5, 2
    H = dv(np.stack([-3.0 * np.eye(D + 1), np.eye(D + 1)]))
    g, trial = dv(np.ones((L, D + 1))), dv(np.zeros((L, D + 1)))
    state = dv(state_of([1, 1]))
    delta, dec = f64(L, D + 1), f64(L)
    po.prop_solve(H, g, trial, 0, 1.0, state, delta, dec)
    st = state.cpu().numpy()
    want = ms.host_solve(-3.0 * np.eye(D + 1), np.ones(D + 1), np.zeros(D + 1), 1.0)
    assert st[0, po.BAD] == want[2] == D + 1 and st[1, po.BAD] == 0
    ok = ms.host_solve(np.eye(D + 1), np.ones(D + 1), np.zeros(D + 1), 1.0)
    assert np.array_equal(delta[1].cpu().numpy(), ok[0]) and float(dec[1]) == ok[1]
    assert np.array_equal(delta[0].cpu().numpy(), want[0], equal_nan=True)


# ---------------------------------------------------------------------------------- the whole fit
@functools.lru_cache(maxsize=None)
def fit_case(kind, n, D):
    X, y = ref.make_data(kind, n, D, 1)
    return X, y, ref.newton(X, y), LabPropensity(C=1.0, max_iter=50, tol=TOL).fit(X, y[:, None])


def distance(p, j, w, b):
    return max(float(np.abs(p.coef_[j] - w).max()), abs(float(p.intercept_[j] - b)))


@functools.lru_cache(maxsize=None)
def device_fit(kind, n, D):
    X, y, _, _ = fit_case(kind, n, D)
    Y = np.stack([y, np.zeros_like(y), np.ones_like(y)], axis=1)                       # and the two degenerate labs
    return LabPropensity(C=1.0, max_iter=50, tol=TOL).fit(padded(X), dv(Y))


@pytest.mark.parametrize("kind, n, D", ref.CASES)
def test_the_device_fit_meets_the_80_bit_newton(kind, n, D):
    X, y, (w, b), host = fit_case(kind, n, D)
    dev = device_fit(kind, n, D)
    d = distance(dev, 0, w, b)
    print(f"{kind} n {n} D {D}: device distance {d:.2e}, host {distance(host, 0, w, b):.2e}, n_iter {dev.n_iter_[0]} / "
          f"{host.n_iter_[0]}, last decrement {dev.decrement_[0]:.2e} of {TOL * n:.2e}")
    assert dev.converged_[0] and d <= 8 * HOST_DISTANCE
    assert dev.degenerate_.tolist() == [False, True, True] and dev.n_iter_[1] == dev.n_iter_[2] == 0
    assert not dev.coef_[1:].any() and dev.intercept_[1] == -np.inf and dev.intercept_[2] == np.inf
    prob = dev.predict_proba(padded(X)).cpu().numpy()
    assert np.all(prob[:, 1] == 0.0) and np.all(prob[:, 2] == 1.0)
    assert np.isclose(dev.pseudo_r2_[0], host.pseudo_r2_[0], rtol=1e-9) and np.isclose(dev.brier_[0], host.brier_[0], rtol=1e-9)
    assert np.isnan(dev.pseudo_r2_[1]) and dev.brier_[2] == 0.0


def test_the_device_takes_the_hosts_iterations_on_the_twelve_cases():
    """n_iter_ and the halvings equal the host's wherever the last decrement is not within a factor 2 of tol * n (there
    rounding may cross the stop); at most two of the twelve cases may be exempted by that."""
    exempt = []
    for kind, n, D in ref.CASES:
        host, dev = fit_case(kind, n, D)[3], device_fit(kind, n, D)
        if TOL * n / 2 <= min(dev.decrement_[0], host.decrement_[0]):
            exempt.append((kind, n, D))
        else:
            assert dev.n_iter_[0] == host.n_iter_[0] and dev.halvings_[0] == host.halvings_[0], (kind, n, D)
    print(f"exempted: {exempt}")
    assert len(exempt) <= 2


def many_labs(n, D, L):
    rng = np.random.default_rng(L)
    X = rng.standard_normal((n, D)).astype(F32)
    W = rng.standard_normal((D, L))
    Y = (X.astype(np.float64) @ W + rng.logistic(size=(n, L)) + np.linspace(-2, 2, L)[None, :] > 0).astype(np.uint8)
    return X, Y


@pytest.mark.parametrize("L", [1, 3, 64, 65])
def test_every_batch_size_meets_the_host_path(L):
    assert po.prop_batch(300, 3) == 64
    X, Y = many_labs(300, 3, L)
    host = LabPropensity(tol=TOL, max_iter=40).fit(X, Y)
    dev = LabPropensity(tol=TOL, max_iter=40).fit(padded(X), dv(Y))
    assert dev.converged_.all() and host.converged_.all()
    assert float(np.abs(dev.coef_ - host.coef_).max()) <= 8 * HOST_DISTANCE
    assert float(np.abs(dev.intercept_ - host.intercept_).max()) <= 8 * HOST_DISTANCE
    gap = np.minimum(dev.decrement_, host.decrement_) < TOL * 300 / 2
    assert L - gap.sum() <= (0 if L <= 3 else 2), "labs exempted from the n_iter_ comparison: none at 1 and 3 labs, at most two"
    assert np.array_equal(dev.n_iter_[gap], host.n_iter_[gap])


def new_fit(X, Y, max_iter=12, tol=TOL):
    n, D = X.shape
    trial, state, _ = ms.start_point(Y.sum(0), n, D)
    return ms._DeviceFit(padded(X), dv(X.astype(np.float64).mean(0)), dv(Y), trial, state, 1.0, tol * n, max_iter)


def test_a_lab_frozen_early_does_not_change_while_the_others_go_on():
    X, Y = many_labs(300, 3, 5)
    Y[:, 1] = X[:, 0] > 0                                    # a slow lab among quick ones
    fit = new_fit(X, Y, max_iter=20)
    frozen = {}
    names = ("beta", "trial", "step", "fstate", "state")
    for r in range(21):
        fit.round()
        st = fit.state.cpu().numpy()
        for j in np.flatnonzero(st[:, ms.ACTIVE] == 0):
            rows = [bits(getattr(fit, nm)[j]).clone() if nm != "state" else getattr(fit, nm)[j].clone() for nm in names]
            if j in frozen:
                assert all(torch.equal(a, b) for a, b in zip(frozen[j][1], rows)), (j, r)
            else:
                frozen[int(j)] = (r, rows)
    assert len(frozen) == 5 and len({r for r, _ in frozen.values()}) > 1, "the labs freeze in different rounds"


def test_the_fit_is_bitwise_the_same_eager_repeated_and_as_a_replayed_capture():
    X, Y = many_labs(300, 17, 4)
    a = LabPropensity(tol=TOL).fit(padded(X), dv(Y))
    b = LabPropensity(tol=TOL).fit(padded(X), dv(Y))
    assert np.array_equal(a.coef_, b.coef_) and np.array_equal(a.intercept_, b.intercept_) and np.array_equal(a.n_iter_, b.n_iter_)
    rounds = 13
    eager = new_fit(X, Y)
    for _ in range(rounds):
        eager.round()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        new_fit(X, Y).round()                                 # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    captured = new_fit(X, Y)
    start = {nm: getattr(captured, nm).clone() for nm in ("beta", "trial", "step", "fstate", "state")}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.round()                                      # one Newton step: link, moments, solve, update
    for nm, t in start.items():
        getattr(captured, nm).copy_(t)
    for _ in range(rounds):
        graph.replay()
    torch.cuda.synchronize()
    for nm in ("beta", "trial", "step", "fstate"):
        assert torch.equal(bits(getattr(captured, nm)), bits(getattr(eager, nm))), nm
    assert torch.equal(captured.state, eager.state) and int(eager.state[:, po.CONVERGED].sum()) == 4


# ---------------------------------------------------------------------------------- predict
@pytest.mark.parametrize("D, n", [(3, 1), (17, 130), (128, 257)])
def test_predict_proba_on_new_rows_equals_the_restatement(D, n):
    X, Y = many_labs(300, D, 5)
    Y[:, 4] = 0
    fit = LabPropensity(tol=1e-8).fit(padded(X), dv(Y))
    new = np.random.default_rng(n).standard_normal((n, D)).astype(F32) * 1.5
    got = fit.predict_proba(padded(new))
    want = ms.host_predict(new, fit._st["mean"], fit._st["beta"])
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 5)
    assert np.array_equal(got.cpu().numpy(), want), float(np.abs(got.cpu().numpy() - want).max())
    assert np.all(want[:, 4] == 0.0)
    out = torch.full((n, 9), -7.0, dtype=torch.float32, device=DEV)
    po.prop_predict(padded(new), dv(fit._st["mean"]), dv(fit._st["beta"]), out=out[:, :5])
    assert torch.equal(out[:, :5], got) and bool((out[:, 5:] == -7.0).all()), "the padding of a strided output is not written"


# ---------------------------------------------------------------------------------- weighted error sums over pairs
def device_pair_sums(case, clip, stabilized):
    pred, y, pi, li, P, cov = case
    count, sums = po.prop_pair_sums(dv(pred), dv(y), dv(pi), dv(li), padded(P), dv(cov), clip, stabilized)
    return count.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("stabilized", [False, True])
@pytest.mark.parametrize("m, L", [(0, 3), (1, 1), (255, 3), (256, 1), (257, 3), (5000, 50), (3000, 512), (70000, 7)])
def test_pair_sums_equal_the_restatement_in_shuffled_and_lab_major_order(m, L, stabilized):
    for order in ("shuffled", "lab-major"):
        case = ref.pair_case(m, 40, L, m + L, order, empty_lab=1)
        count, sums = device_pair_sums(case, 0.02, stabilized)
        wc, ws = ms.host_pair_sums(*case, 0.02, stabilized)
        assert count.dtype == np.int64 and np.array_equal(count, wc), order
        assert np.array_equal(sums, ws), (order, float(np.abs(sums - ws).max()))
        if L > 1:
            assert count[1] == 0 and not sums[1].any(), "a lab with no pair"
        again = device_pair_sums(case, 0.02, stabilized)
        assert np.array_equal(again[1].view(np.int64), sums.view(np.int64)), "two runs differ"
    a = ref.pair_case(m, 40, L, m + L, "shuffled", empty_lab=1)
    b = ref.pair_case(m, 40, L, m + L, "lab-major", empty_lab=1)
    assert np.array_equal(np.sort(a[3]), b[3])


def test_pair_sums_leave_out_pairs_outside_the_table_and_ipw_metrics_refuses_them():
    case = list(ref.pair_case(700, 40, 5, 3))
    keep = np.ones(700, bool)
    keep[[5, 300, 699]] = False
    want = ms.host_pair_sums(case[0][keep], case[1][keep], case[2][keep], case[3][keep], case[4], case[5], 0.05, True)
    case[3] = case[3].copy(); case[2] = case[2].copy()
    case[3][5], case[3][300], case[2][699] = -1, 5, 40
    count, sums = device_pair_sums(case, 0.05, True)
    assert np.array_equal(count, want[0]) and np.array_equal(sums, want[1])
    with pytest.raises(ValueError, match="outside"):
        ms.ipw_metrics(*(dv(t) for t in case[:5]))


def test_ipw_metrics_on_the_device_are_the_numpy_paths():
    pred, y, pi, li, P, cov = ref.pair_case(5000, 300, 9, 17, empty_lab=4)
    for kw in (dict(), dict(stabilized=False, clip=0.1), dict(coverage=cov)):
        host = ms.ipw_metrics(pred, y, pi, li, P, **kw)
        dev = ms.ipw_metrics(dv(pred), dv(y), dv(pi), dv(li), dv(P), **{k: (dv(v) if k == "coverage" else v) for k, v in kw.items()})
        assert np.array_equal(dev.count, host.count)
        if "coverage" in kw or not kw.get("stabilized", True):
            assert np.array_equal(dev.sums, host.sums)                # the same numerator: EQUAL
        assert np.allclose(dev.sums, host.sums, rtol=1e-12, atol=0)   # the default numerator is a column mean: two orders
        assert dev.per_lab.columns.tolist() == list(ms.IPW_COLUMNS) and dev.overall["n"] == 5000
    one = ms.ipw_metrics(dv(pred), dv(y), dv(pi), dv(li), dv(np.ones_like(P)), stabilized=False)
    assert np.array_equal(one.sums[:, 2], one.sums[:, 4]) and np.array_equal(one.sums[:, 3], one.sums[:, 5])
    assert np.array_equal(one.sums[:, 0], one.count.astype(np.float64))


# ---------------------------------------------------------------------------------- refusals
def test_every_refusal_comes_before_anything_is_enqueued():
    n, D, L = 100, 8, 4
    X, Y = many_labs(n, D, L)
    Xd, Yd, mean = dv(X), dv(Y), dv(X.astype(np.float64).mean(0))
    lib = po.load()
    E_ARG, E_WS = _lib.MMG_E_ARG, _lib.MMG_E_WS
    H, g, sr = f64(L, D + 1, D + 1, fill=-7.0), f64(L, D + 1, fill=-7.0), f64(2, L, n, fill=0.25)
    p = lambda t: t.data_ptr()                                                          # noqa: E731
    need = lib.mmg_prop_moments_ws_bytes(n, D, L)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.mmg_prop_moments(p(Xd), n, D, D, p(mean), p(sr), L, 0, L, None, p(H), p(g), p(ws), need - 1, None) == E_WS
    assert lib.mmg_prop_moments(p(Xd), n, D, D, p(mean), p(sr), L, 0, L, None, p(H), p(g), None, need, None) == E_WS
    assert lib.mmg_prop_moments(p(Xd), n, D, D - 1, p(mean), p(sr), L, 0, L, None, p(H), p(g), p(ws), need, None) == E_ARG
    assert lib.mmg_prop_moments(p(Xd), n, D, D, p(mean), p(sr), L, 2, L, None, p(H), p(g), p(ws), need, None) == E_ARG
    torch.cuda.synchronize()
    assert bool((H == -7.0).all()) and bool((g == -7.0).all())
    with pytest.raises(ValueError):
        po.prop_moments(Xd, mean, sr[:, :2], L, 0, L, None, H, g)
    with pytest.raises(TypeError):
        po.prop_link(Xd, mean, Yd.float(), 0, L, f64(L, D + 1, fill=0.0), None, sr, f64(L, po.link_blocks(n)))
    with pytest.raises(ValueError, match="NaN or infinite"):
        bad = Xd.clone()
        bad[3, 2] = float("nan")
        LabPropensity().fit(bad, Yd)
    with pytest.raises(ValueError, match="both"):
        LabPropensity().fit(Xd, Y)


# ---------------------------------------------------------------------------------- the drivers
def test_the_report_on_the_device_is_the_numpy_paths(tmp_path):
    import pandas as pd
    g = make_graph(1, seed=0)
    Fh, names_h = ms.measurement_features(g, "codes", 16)
    Fd, names_d = ms.measurement_features(g.to(DEV), "codes", 16)
    assert names_h == names_d and Fd.is_cuda and Fd.dtype == torch.float32 and np.array_equal(Fd.cpu().numpy(), Fh)
    ph, fh = ms.missingness_report(g, tmp_path / "host", max_features=16, tol=1e-10)
    pd_, fd = ms.missingness_report(g.to(DEV), tmp_path / "dev", max_features=16, tol=1e-10)
    for name in ("lab_propensity.csv", "lab_propensity_coefficients.csv"):
        a, b = pd.read_csv(tmp_path / "host" / name), pd.read_csv(tmp_path / "dev" / name)
        assert list(a.columns) == list(b.columns) and len(a) == len(b) == int(g["lab"].num_nodes)
    assert float(np.abs(pd_.coef_ - ph.coef_).max()) <= 1e-9 and np.array_equal(pd_.degenerate_, ph.degenerate_)
    fin = ~ph.degenerate_
    assert np.allclose(pd_.intercept_[fin], ph.intercept_[fin], rtol=0, atol=1e-9)
    assert np.allclose(pd_.pseudo_r2_[fin], ph.pseudo_r2_[fin], rtol=0, atol=1e-9) and np.allclose(pd_.brier_, ph.brier_, rtol=0, atol=1e-9)
    assert list(fd["propensity"].columns[:7]) == ["lab", "coverage", "pseudo_r2", "brier", "n_iter", "converged", "degenerate"]
    assert list(fd["coefficients"].columns) == ["lab", "intercept"] + names_d


def test_the_report_with_a_model_writes_the_weighted_errors(tmp_path):
    import pandas as pd
    from mmgnn import conformal as cf
    from mmgnn.model import build_model
    from mmgnn.train import EdgeMasker
    g = make_graph(1, seed=0).to(DEV)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    model._init_embeddings(g)
    masker = EdgeMasker(g)
    prop, frames = ms.missingness_report(g, tmp_path, model=model, masker=masker, split="test", max_features=16, tol=1e-10)
    for name in ("lab_propensity.csv", "lab_propensity_coefficients.csv", "ipw_metrics.csv"):
        assert (tmp_path / name).exists(), name
    L = int(g["lab"].num_nodes)
    table = pd.read_csv(tmp_path / "ipw_metrics.csv")
    assert list(table.columns) == list(ms.IPW_COLUMNS) and len(table) == L + 1 and table["lab"].iloc[-1] == "overall"
    # the numpy path on the same predictions and propensities
    _, pred, y, pi, li = cf._predict_split(model, g, masker, "test")
    feats, _ = ms.measurement_features(g, "codes", 16)
    P = prop.predict_proba(feats).cpu().numpy()
    host = ms.ipw_metrics(pred.cpu().numpy(), y.cpu().numpy(), pi.cpu().numpy(), li.cpu().numpy(), P, coverage=prop.coverage_)
    assert int(table["n"].iloc[-1]) == host.overall["n"] == int(masker.test_mask.sum())
    assert np.array_equal(table["n"].to_numpy()[:L], host.per_lab["n"].to_numpy())
    for k in ms.IPW_COLUMNS[2:]:
        want = np.append(host.per_lab[k].to_numpy(), host.overall[k])
        assert np.allclose(table[k].to_numpy(), want, rtol=1e-12, atol=0, equal_nan=True), k
    assert np.all(table["ess"].to_numpy()[:L] <= table["n"].to_numpy()[:L] * (1 + 1e-12))
    with pytest.raises(ValueError, match="both the model and the masker"):
        ms.missingness_report(g, tmp_path, model=model)


def test_planted_coefficients_come_back_and_constant_rate_labs_explain_nothing():
    """Labels drawn from known coefficients over the code features of synth.make_graph x1: the sign of every planted
    coefficient with |w| >= 0.5 comes back and those labs have pseudo-R^2 > 0; labs drawn at a constant rate stay within
    +-0.01 of 0 (thresholds checked with the numpy path first: tests/test_missingness_cpu.py has the same case)."""
    from test_missingness_cpu import planted
    F, Y, W, flat = planted()
    fit = LabPropensity(tol=1e-10).fit(dv(F), dv(Y))
    big = np.abs(W) >= 0.5
    assert big.sum() >= 6 and np.array_equal(np.sign(fit.coef_.T[big]), np.sign(W[big]))
    assert np.all(fit.pseudo_r2_[~flat] > 0.0) and np.all(np.abs(fit.pseudo_r2_[flat]) <= 0.01)
