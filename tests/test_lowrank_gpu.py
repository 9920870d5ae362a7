"""Low-rank lab imputation on the MI355X (libmmgnn_mf.so through mmgnn/mf_ops.py): the sums of a half-sweep, read
through normal_out, EQUAL the loop reference (tests/mf_ref.py) on lattice inputs and sit inside the derived bound on
generic ones, at every rank where the entries per lane change and every segment length where the launch plan switches;
exact symmetry; the same bits wherever a segment lies; bitwise repeatability; the solve, the predictions, impute_matrix
and the index EQUAL the numpy restatement on the device's own inputs; centre and objective follow the sum rule; the whole
fit against the 80-bit chain with the host path's distance as the yardstick; one captured round replayed; every refusal
before anything is enqueued; the drivers, device against the numpy path."""
import functools

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib
from mmgnn import evaluate as ev
from mmgnn import lowrank as lr
from mmgnn import mf_ops as mo
from mmgnn.lowrank import LowRankLabImputer
from mmgnn.model import build_model
from mmgnn.synth import make_graph
from mmgnn.train import EdgeMasker
import mf_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
CH = mo.MF_CHUNK
RANKS = (1, 2, 3, 8, 15, 16, 17, 32)
OTHERS = (1, 50, 2048)


def dv(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def plan_switches():
    """The lengths at which mmg_mf_plan changes its path, read from the plan function itself."""
    paths = [mo.mf_plan(n)[0] for n in range(0, 4 * mo.MF_SPLIT + 2)]
    return [n for n in range(1, len(paths)) if paths[n] != paths[n - 1]]


@functools.lru_cache(maxsize=None)
def lengths():
    """0, 1, 2, a chunk minus, exactly and plus one pair, two chunks and 77; the last length of every path, the first of
    the next; one long enough to be split into many ragged chunks."""
    sw = plan_switches()
    assert sw == [1, mo.MF_SPLIT + 1] and mo.MF_SPLIT % CH == 0 and ref.CHUNK == CH
    out = [0, 1, 2, CH - 1, CH, CH + 1, 2 * CH + 77]
    for n in sw[1:]:
        out += [n - 1, n]
    out += [0, 2 * mo.MF_SPLIT + 3 * CH + 5, 33]
    assert [mo.mf_plan(n)[0] for n in out[-3:]] == [mo.MMG_MF_PATH_EMPTY, mo.MMG_MF_PATH_SPLIT, mo.MMG_MF_PATH_WAVE]
    return tuple(out)


def device_sweep(ptr, idx, y, F, reg):
    """-> (A [S, r, r], b [S, r], x [S, r], bad) of one mmg_mf_half_sweep with normal_out."""
    S, r = len(ptr) - 1, F.shape[1]
    out = torch.full((S, r), -7.0, dtype=torch.float64, device=DEV)
    normal = torch.full((S, r * r + r), -7.0, dtype=torch.float64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int64, device=DEV)
    mo.mf_half_sweep(dv(ptr), dv(idx), dv(y), dv(F), reg, out, bad, normal_out=normal)
    n = normal.cpu().numpy()
    return n[:, :r * r].reshape(S, r, r), n[:, r * r:], out.cpu().numpy(), int(bad.item())


@functools.lru_cache(maxsize=None)
def sweep_case(r, m, lattice):
    ptr, idx, y, F = ref.make_segments(lengths(), m, r, seed=100 * r + m, lattice=lattice)
    return ptr, idx, y, F, ref.normal(ptr, idx, y, F, 0.5)


# ---------------------------------------------------------------------------------- the sums of a half-sweep
@pytest.mark.parametrize("m", OTHERS)
@pytest.mark.parametrize("r", RANKS)
def test_lattice_sums_equal_the_loop_reference(r, m):
    ptr, idx, y, F, (wA, wb, _, _) = sweep_case(r, m, True)
    A, b, x, bad = device_sweep(ptr, idx, y, F, 0.5)
    assert np.array_equal(A, wA) and np.array_equal(b, wb) and bad == 0
    xs, _ = lr.host_solve(A, b)
    xs[np.diff(ptr) == 0] = 0.0
    assert np.array_equal(x, xs), "the solve EQUALS the restatement on the device's own A | b"


@pytest.mark.parametrize("m", OTHERS)
@pytest.mark.parametrize("r", RANKS)
def test_generic_sums_are_inside_the_bound_symmetric_placed_anywhere_and_repeatable(r, m):
    ptr, idx, y, F, (wA, wb, Aa, ba) = sweep_case(r, m, False)
    A, b, x, bad = device_sweep(ptr, idx, y, F, 0.5)
    n = np.diff(ptr)
    errA, errb = np.abs(A - wA) / np.maximum(ref.sum_bound(n[:, None, None], Aa), 1e-300), \
        np.abs(b - wb) / np.maximum(ref.sum_bound(n[:, None], ba), 1e-300)
    print(f"rank {r}, other {m}: largest error {max(errA.max(), errb.max()):.3f} of the bound")
    assert errA.max() <= 1.0 and errb.max() <= 1.0
    assert np.array_equal(A, A.transpose(0, 2, 1)), "exactly symmetric"
    xs, nb = lr.host_solve(A, b)
    xs[n == 0] = 0.0
    assert np.array_equal(x, xs) and bad == nb == 0
    A2, b2, x2, _ = device_sweep(ptr, idx, y, F, 0.5)
    assert np.array_equal(A, A2) and np.array_equal(b, b2) and np.array_equal(x, x2), "two runs, the same bits"
    # the same segments in the reverse order: every one at another offset, among other neighbours
    S = len(n)
    rev = np.arange(S)[::-1]
    pieces = [(idx[ptr[s]:ptr[s + 1]], y[ptr[s]:ptr[s + 1]]) for s in rev]
    ptr_r = np.concatenate([[0], np.cumsum(n[rev])]).astype(np.int64)
    A3, b3, x3, _ = device_sweep(ptr_r, np.concatenate([p[0] for p in pieces]), np.concatenate([p[1] for p in pieces]), F, 0.5)
    assert np.array_equal(A3[::-1], A) and np.array_equal(b3[::-1], b) and np.array_equal(x3[::-1], x)


def test_the_production_call_without_normal_out_gives_the_same_vectors():
    ptr, idx, y, F, _ = sweep_case(8, 50, False)
    _, _, x, _ = device_sweep(ptr, idx, y, F, 0.5)
    out = torch.full((len(ptr) - 1, 8), -7.0, dtype=torch.float64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int64, device=DEV)
    mo.mf_half_sweep(dv(ptr), dv(idx), dv(y), dv(F), 0.5, out, bad)
    assert np.array_equal(out.cpu().numpy(), x) and int(bad.item()) == 0
    assert not x[np.diff(ptr) == 0].any(), "an empty segment gets the zero vector"


def test_a_pivot_that_is_not_positive_is_counted():
    """A hand-made system whose Cholesky breaks down: one pair with the factor row (1e200, 1e200, 1e200) makes every
    entry of A infinite, the first column inf / inf = NaN, and the two pivots after the first are NaN: not > 0.  A
    second, ordinary segment beside it is untouched."""
    F = np.array([[1e200, 1e200, 1e200], [0.5, -1.0, 2.0]])
    ptr, idx, y = np.array([0, 1, 3], np.int64), np.array([0, 1, 1], np.int32), np.array([1.0, 2.0, -1.0])
    with np.errstate(all="ignore"):
        A, b, x, bad = device_sweep(ptr, idx, y, F, 1.0)
        xs, nb = lr.host_solve(A, b)
    assert np.isinf(A[0]).all() and bad == nb == 2
    assert np.array_equal(x, xs, equal_nan=True) and np.isnan(x[0]).all() and np.isfinite(x[1]).all()


# ---------------------------------------------------------------------------------- the index
@pytest.mark.parametrize("n, L, density", [(700, 5, 0.9), (3000, 50, 0.3), (1, 1, 1.0), (40, 2048, 0.02), (5, 3, 0.0)])
def test_the_index_equals_numpys_stable_sorts_and_the_centre_follows_the_sum_rule(n, L, density):
    p, lab, v = ref.make_triples(n, L, density, seed=n + L, empty_lab=1 if L > 2 else None)
    ix = mo.mf_index(dv(p), dv(lab), dv(v), n, L)
    h = lr.host_index(p, lab, v, n, L)
    for k in ("p_ptr", "p_idx", "l_ptr", "l_idx", "count"):
        assert np.array_equal(getattr(ix, k).cpu().numpy(), h[k]), k
    assert np.array_equal(ix.p_val.cpu().numpy().view(np.int32), h["p_val"].view(np.int32))
    center = ix.center.cpu().numpy()
    ol = np.lexsort((p, lab))
    vl, ll = v[ol].astype(np.float64), lab[ol]
    for l in range(L):
        want = ref.rule_sum(vl[ll == l]) / h["count"][l] if h["count"][l] else 0.0
        assert center[l] == want, l
    assert np.array_equal(ix.l_y.cpu().numpy(), vl - center[ll])
    op = np.lexsort((lab, p))
    assert np.array_equal(ix.p_y.cpu().numpy(), v[op].astype(np.float64) - center[lab[op]])
    if p.size:
        assert h["count"].max() > CH or n < CH, "a lab longer than a chunk where the shape allows one"
        fixed = np.linspace(-1.0, 1.0, L)
        ix2 = mo.mf_index(dv(p), dv(lab), dv(v), n, L, center=dv(fixed))
        assert np.array_equal(ix2.center.cpu().numpy(), fixed) and np.array_equal(ix2.count.cpu().numpy(), h["count"])
        assert np.array_equal(ix2.p_y.cpu().numpy(), v[op].astype(np.float64) - fixed[lab[op]])


# ---------------------------------------------------------------------------------- objective, predictions
@pytest.mark.parametrize("n, L, r, density", [(300, 20, 4, 0.3), (1400, 50, 16, 0.95), (3, 2, 1, 0.0)])
def test_the_objective_follows_the_sum_rule(n, L, r, density):
    """The items -- (y - u.v)^2 pair by pair in the by-patient order, the squares of U and of V row-major -- are the
    restatement's, bit for bit; their sums are the rule's, level after level ((1400, 50): more than CHUNK^2 pairs)."""
    p, lab, v = ref.make_triples(n, L, density, seed=n)
    rng = np.random.default_rng(n)
    U, V = rng.standard_normal((n, r)), rng.standard_normal((L, r))
    ix = mo.mf_index(dv(p), dv(lab), dv(v), n, L)
    out = torch.full((3,), -7.0, dtype=torch.float64, device=DEV)
    mo.mf_objective(ix, dv(U), dv(V), out)
    h = lr.host_index(p, lab, v, n, L)
    h["p_y"] = ix.p_y.cpu().numpy()
    pat = np.repeat(np.arange(n), np.diff(h["p_ptr"]))
    d = h["p_y"] - lr._dots(U[pat], V[h["p_idx"].astype(np.int64)])
    want = [ref.rule_sum_levels(d * d), ref.rule_sum_levels((U * U).ravel()), ref.rule_sum_levels((V * V).ravel())]
    assert out.cpu().numpy().tolist() == want
    if density > 0.9:
        assert p.size > CH * CH
    loose = lr.host_objective(h, U, V)
    assert np.allclose(want, loose, rtol=1e-12, atol=0)


@functools.lru_cache(maxsize=None)
def device_fit(n=257, L=17, rank=4, lo=-np.inf, hi=np.inf):
    p, lab, v = ref.make_triples(n, L, 0.3, seed=n + L, empty_lab=2)
    imp = LowRankLabImputer(rank=rank, reg=1.0, tol=0, max_iter=3, seed=5, min_value=lo, max_value=hi)
    return p, lab, v, imp.fit(dv(p), dv(lab), dv(v), n, L)


@pytest.mark.parametrize("lo, hi", [(-np.inf, np.inf), (0.5, 3.0)])
def test_predictions_and_impute_matrix_equal_the_restatement_on_the_devices_factors(lo, hi):
    n, L = 257, 17
    p, lab, v, imp = device_fit(lo=lo, hi=hi)
    U, V = imp.patient_factors_.cpu().numpy(), imp.lab_factors_.cpu().numpy()
    st = imp._state
    assert np.array_equal(V, st["V"]) and imp.patient_factors_.is_cuda
    h = lr.host_index(p, lab, v, n, L)
    out = imp.impute_matrix()
    want = lr.host_impute(None, U, V, st["center"], st["count"], lo, hi, h)
    assert out.is_cuda and out.dtype == torch.float32
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.isnan(want[:, 2]).all() and np.array_equal(want[p, lab].view(np.int32), v.view(np.int32))
    if np.isfinite(lo):
        miss = np.ones((n, L), bool)
        miss[p, lab] = False
        miss[:, 2] = False
        assert (want[miss] == F32(lo)).any() and (want[miss] == F32(hi)).any() and ((want[miss] > lo) & (want[miss] < hi)).any()
    rows = np.array([3, 0, n - 1, 3])
    assert torch.equal(bits(imp.impute_matrix(dv(rows))), bits(out[dv(rows)]))
    rng = np.random.default_rng(1)
    qp, ql = rng.integers(0, n, 999), rng.integers(0, L, 999)
    got = imp.predict(dv(qp), dv(ql)).cpu().numpy()
    assert np.array_equal(got.view(np.int32), lr.host_predict(qp, ql, U, V, st["center"], st["count"], lo, hi).view(np.int32))
    assert np.isnan(got[ql == 2]).all() and not np.isnan(got[ql != 2]).any()


# ---------------------------------------------------------------------------------- the whole fit
@functools.lru_cache(maxsize=None)
def chain_case(n, L, rank):
    p, lab, v = ref.make_triples(n, L, 0.3, seed=n + L, empty_lab=2)
    host = LowRankLabImputer(rank=rank, reg=1.0, tol=0, max_iter=3, seed=5).fit(p, lab, v, n, L)
    V0 = np.random.default_rng(5).standard_normal((L, rank)) * 0.1
    return p, lab, v, host, ref.als(p, lab, v, n, L, V0, 1.0, 3)


@pytest.mark.parametrize("n, L, rank", [(257, 17, 4), (1000, 50, 16)])
def test_the_whole_fit_against_the_80_bit_chain(n, L, rank):
    """Three rounds, tol = 0: the device is at most 8 x as far from the 80-bit chain as the host path is.
    Measured on an MI355X: see DESIGN.md section 5, "Low-rank imputation"."""
    p, lab, v, host, (Uw, Vw, hist, _) = chain_case(n, L, rank)
    imp = LowRankLabImputer(rank=rank, reg=1.0, tol=0, max_iter=3, seed=5).fit(dv(p), dv(lab), dv(v), n, L)
    dist = lambda U, V: max(float(np.abs(U.astype(ref.LD) - Uw).max()), float(np.abs(V.astype(ref.LD) - Vw).max()))   # noqa: E731
    d_dev = dist(imp.patient_factors_.cpu().numpy(), imp.lab_factors_.cpu().numpy())
    d_host = dist(host.patient_factors_, host.lab_factors_)
    print(f"({n}, {L}) rank {rank}: device {d_dev:.2e}, host path {d_host:.2e} from the 80-bit chain, "
          f"ratio {d_dev / d_host:.2f}")
    assert d_host > 0 and d_dev <= 8 * d_host
    assert imp.n_iter_ == host.n_iter_ == 3 and np.allclose(imp.history_, host.history_, rtol=1e-9, atol=0)
    assert np.allclose(imp.history_, hist, rtol=1e-9, atol=0)
    out = imp.impute_matrix()
    # transform of the training triples is bitwise the fit; new patients EQUAL the host path on the device's factors
    assert torch.equal(bits(imp.transform(dv(p), dv(lab), dv(v), n)), bits(out))
    pn, ln, vn = ref.make_triples(77, L, 0.5, seed=9 * n + L)
    got = imp.transform(dv(pn), dv(ln), dv(vn), 77).cpu().numpy()
    other = LowRankLabImputer().load_state_dict(imp.state_dict())
    ixn = mo.mf_index(dv(pn), dv(ln), dv(vn), 77, L, center=imp._dev[DEV]["center"])
    A, b, x, _ = device_sweep(ixn.p_ptr.cpu().numpy(), ixn.p_idx.cpu().numpy(), ixn.p_y.cpu().numpy(), imp._state["V"], 1.0)
    hn = lr.host_index(pn, ln, vn, 77, L, center=imp._state["center"])
    want = lr.host_impute(None, x, imp._state["V"], imp._state["center"], imp._state["count"], -np.inf, np.inf, hn)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # a state loaded elsewhere transforms on the device without the training data
    assert torch.equal(bits(other.transform(dv(p), dv(lab), dv(v), n)), bits(out))
    with pytest.raises(RuntimeError, match="transform"):
        other.impute_matrix()


def test_the_stopping_rule_on_the_device():
    p, lab, v = ref.make_triples(120, 9, 0.4, seed=21, empty_lab=6)
    kw = dict(rank=3, reg=0.7, max_iter=12)
    h = LowRankLabImputer(tol=0, **kw).fit(p, lab, v, 120, 9).history_
    rel = [(h[i - 1] - h[i]) / h[i - 1] for i in range(1, 12)]
    k = next(i for i in range(1, 11) if rel[i] < rel[i - 1] / 1.5 and all(x > rel[i] * 1.2 for x in rel[:i]))
    tol = float(np.sqrt(rel[k] * min(rel[:k])))
    assert min(rel[:k]) > 1.2 * tol and rel[k] < tol / 1.2, "an asserted gap: rounding cannot cross it"
    imp = LowRankLabImputer(tol=tol, **kw).fit(dv(p), dv(lab), dv(v), 120, 9)
    assert imp.n_iter_ == k + 2 and np.allclose(imp.history_, h[:k + 2], rtol=1e-9, atol=0)


def test_a_replayed_captured_round_is_bitwise_the_eager_round():
    """One round -- two half-sweeps (wave and split paths: lab 0 has more than MMG_MF_SPLIT patients) and the objective
    -- in ONE captured hipGraph (no allocation, no memset node, no host synchronisation inside), one replay."""
    n, L, r = 2600, 6, 4
    p, lab, v = ref.make_triples(n, L, 0.9, seed=4)
    ix = mo.mf_index(dv(p), dv(lab), dv(v), n, L)
    assert int(ix.count.max()) > mo.MF_SPLIT
    V0 = np.random.default_rng(2).standard_normal((L, r)) * 0.1

    def new_als():
        return lr._DeviceALS(ix, dv(V0), 1.0, 1)

    eager = new_als()
    eager.round(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        new_als().round(0)                                   # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    captured = new_als()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.round(0)
    captured.V.copy_(dv(V0))
    captured.U.fill_(-1)
    captured.obj.fill_(-1)
    captured.bad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name in ("U", "V", "obj", "bad"):
        assert torch.equal(bits(getattr(captured, name)), bits(getattr(eager, name))), name
    assert float(eager.obj[0, 0]) > 0 and int(eager.bad) == 0
    hU, _ = lr.host_half_sweep(*(t.cpu().numpy() for t in (ix.p_ptr, ix.p_idx, ix.p_y)), V0, 1.0)
    assert np.allclose(eager.U.cpu().numpy(), hU, rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------------------- refusals
def test_every_refusal_comes_before_anything_is_enqueued():
    n, L, r = 100, 8, 4
    p, lab, v = ref.make_triples(n, L, 0.5, seed=0)
    pd_, ld_, vd_ = dv(p), dv(lab), dv(v)
    ix = mo.mf_index(pd_, ld_, vd_, n, L)
    nnz = ix.nnz
    lib = mo.load()
    E_ARG, E_WS = _lib.MMG_E_ARG, _lib.MMG_E_WS
    f64 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=DEV)      # noqa: E731
    U, V, out3, bad = f64(n, r), f64(L, r), f64(3), torch.full((1,), -7, dtype=torch.int64, device=DEV)
    normal = f64(n, r * r + r)
    pred = torch.full((nnz,), -7.0, dtype=torch.float32, device=DEV)
    dense = torch.full((n, L), -7.0, dtype=torch.float32, device=DEV)
    other = torch.zeros(L, r, dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    need = lib.mmg_mf_half_sweep_ws_bytes(n, nnz, r)
    assert 64 < need < ws.numel()
    a = lambda t: t.data_ptr()                                                          # noqa: E731

    def sweep(seg=n, nnz_=nnz, m=L, r_=r, reg=1.0, w=ws.data_ptr(), nbytes=ws.numel(), ptr=a(ix.p_ptr)):
        return lib.mmg_mf_half_sweep(ptr, a(ix.p_idx), a(ix.p_y), seg, nnz_, a(other), m, r_, reg, a(U), a(bad), a(normal),
                                     w, nbytes, st)

    for kw in (dict(seg=0), dict(nnz_=-1), dict(m=0), dict(r_=0), dict(r_=33), dict(reg=0.0), dict(reg=-2.0),
               dict(reg=float("inf")), dict(reg=float("nan")), dict(ptr=None)):
        assert sweep(**kw) == E_ARG, kw
    assert sweep(w=ws.data_ptr(), nbytes=64) == E_WS and sweep(w=None, nbytes=0) == E_WS and sweep(nbytes=need - 1) == E_WS

    def objective(L_=L, r_=r, w=ws.data_ptr(), nbytes=ws.numel(), u=a(U)):
        return lib.mmg_mf_objective(a(ix.p_ptr), a(ix.p_idx), a(ix.p_y), nnz, n, L_, u, a(V), r_, a(out3), w, nbytes, st)

    assert objective(L_=0) == E_ARG and objective(L_=2049) == E_ARG and objective(r_=0) == E_ARG and objective(r_=33) == E_ARG
    assert objective(u=None) == E_ARG and objective(nbytes=64) == E_WS and objective(w=None, nbytes=0) == E_WS

    def index(P=n, L_=L, w=ws.data_ptr(), nbytes=ws.numel(), c=a(ix.count)):
        return lib.mmg_mf_index(a(pd_), a(ld_), a(vd_), nnz, P, L_, None, a(U), a(pred), a(pred), a(normal), a(V), a(pred),
                                a(normal), c, a(out3), w, nbytes, st)

    assert index(P=0) == E_ARG and index(L_=0) == E_ARG and index(L_=2049) == E_ARG and index(c=None) == E_ARG
    assert index(nbytes=64) == E_WS
    cnt, cen = ix.count, ix.center
    pp = lambda L_=L, r_=r, lo=-1.0, hi=1.0, o=a(pred): lib.mmg_mf_predict_pairs(                          # noqa: E731
        a(pd_), a(ld_), nnz, a(U), n, a(V), L_, r_, a(cen), a(cnt), lo, hi, o, st)
    assert pp(L_=0) == E_ARG and pp(r_=33) == E_ARG and pp(lo=1.0) == E_ARG and pp(o=None) == E_ARG
    im = lambda L_=L, r_=r, ld=L, lo=-1.0, hi=1.0: lib.mmg_mf_impute_matrix(                                # noqa: E731
        None, n, a(U), n, a(V), L_, r_, a(cen), a(cnt), lo, hi, a(ix.p_ptr), a(ix.p_idx), a(ix.p_val), nnz, a(dense), ld, st)
    assert im(L_=0) == E_ARG and im(r_=0) == E_ARG and im(ld=L - 1) == E_ARG and im(hi=-1.0) == E_ARG
    torch.cuda.synchronize()
    for t in (U, V, out3, bad, normal, pred, dense):
        assert bool((t == -7).all()), "a refused call wrote something"
    with pytest.raises(_lib.MmgError, match="device tensor"):                # never the host path for host data
        mo.mf_index(torch.from_numpy(p), torch.from_numpy(lab), torch.from_numpy(v), n, L)
    with pytest.raises(ValueError, match="n_labs"):
        LowRankLabImputer().fit(dv(p), dv(lab), dv(v), n, 2049)
    with pytest.raises(ValueError, match="different devices"):
        LowRankLabImputer().fit(dv(p), torch.from_numpy(lab), dv(v), n, L)
    assert sweep() == 0 and objective() == 0 and pp() == 0 and im() == 0     # and the same calls with nothing wrong run
    torch.cuda.synchronize()
    assert not bool((U == -7).any()) and not bool((out3 == -7).any()) and not bool((pred == -7).any())
    assert not bool((dense == -7).any())


# ---------------------------------------------------------------------------------- the drivers
def ulp32(x):
    return np.abs(np.asarray(x, np.float64)) * 2.0 ** -23 + 2.0 ** -149


def test_the_drivers_device_against_the_numpy_path(tmp_path):
    """The fp32 cells of the two paths are the one rounding of two fp64 fits 1e-12 apart: at most one fp32 ulp apart,
    and a mean absolute error over them moves by no more than the largest such ulp."""
    from mmgnn import bootstrap as bt
    g = make_graph(1, seed=0)
    gd = make_graph(1, seed=0).to(DEV)
    kw = dict(rank=4, max_iter=3, tol=0.0)
    host = ev.evaluate_lowrank_baseline(g, EdgeMasker(g), "test", **kw)["low_rank"]
    masker = EdgeMasker(gd)
    dev = ev.evaluate_lowrank_baseline(gd, masker, "test", **kw)["low_rank"]
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    tr_ei, tr_v, _, _ = masker.get_masked_data("train", want_mask=False)
    te_ei, te_v, _, _ = masker.get_masked_data("test", want_mask=False)
    tr_ei, tr_v, te_ei = tr_ei.to(DEV), tr_v.to(DEV).reshape(-1).float(), te_ei.to(DEV)
    host_triples = (tr_ei[0].cpu().numpy(), tr_ei[1].cpu().numpy(), tr_v.cpu().numpy())
    d_imp = LowRankLabImputer(**kw).fit(tr_ei[0], tr_ei[1], tr_v, P, L)
    h_imp = LowRankLabImputer(**kw).fit(*host_triples, P, L)
    a, b = d_imp.impute_matrix().cpu().numpy(), h_imp.impute_matrix()
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(b)] <= ulp32(b)[~np.isnan(b)])
    top = float(ulp32(np.nanmax(np.abs(b))))
    print(f"synthetic x1, test split: low_rank MAE device {dev['mae']:.6f} host {host['mae']:.6f}")
    y = te_v.cpu().numpy().reshape(-1)
    assert dev == ev.compute_regression_metrics(d_imp.predict(te_ei[0], te_ei[1]).cpu().numpy(), y)
    assert host == ev.compute_regression_metrics(h_imp.predict(te_ei[0].cpu().numpy(), te_ei[1].cpu().numpy()), y)
    assert set(dev) == set(host) and abs(dev["mae"] - host["mae"]) <= top
    fitted_ = ev.fit_baselines(("per_lab_mean", "low_rank"), tr_ei, tr_v, L, P)
    kind, (imp, g_mean) = fitted_["low_rank"]
    assert kind == "low_rank" and imp.patient_factors_.is_cuda
    full = LowRankLabImputer().fit(*host_triples, P, L)
    pairs = ev.baseline_pairs(fitted_["low_rank"], te_ei[0], te_ei[1])
    want_pairs = full.predict(te_ei[0].cpu().numpy(), te_ei[1].cpu().numpy())
    assert pairs.is_cuda and imp.n_iter_ == full.n_iter_
    assert np.all(np.abs(pairs.cpu().numpy() - want_pairs) <= ulp32(want_pairs))
    rows = torch.tensor([0, 5, P - 1], device=DEV)
    dense = ev.baseline_matrix(fitted_["low_rank"], rows, L)
    assert dense.shape == (3, L) and torch.equal(dense, torch.where(torch.isnan(imp.impute_matrix(rows)), g_mean,
                                                                    imp.impute_matrix(rows)))
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}, "evaluation": {"stratify_by": []}}
    torch.manual_seed(0)
    model = build_model(cfg, (gd.node_types, gd.edge_types), None).to(DEV)
    model._init_embeddings(gd)
    out = bt.evaluate_with_intervals(model, gd, masker, cfg, tmp_path, replicates=20, baselines=("low_rank",))
    rows = {(r["baseline"], r["metric"]): r for r in out["baseline_comparison"]}
    assert {k[0] for k in rows} == {"low_rank"}
    model_mae = out["overall"][0]["estimate"]
    want = float(np.abs(want_pairs.astype(np.float64) - y.astype(np.float64)).mean())
    got = model_mae - rows[("low_rank", "mae")]["estimate"]
    assert abs(got - want) <= top + 1e-6 * want              # 1e-6: the allowance test_bootstrap_gpu gives this estimate
