"""Low-rank lab imputation without a GPU: the numpy restatement of mmgnn/lowrank.py against the loop reference of
tests/mf_ref.py (sums EQUAL on lattice input, the solve inside its stated rounding, the whole chain against the 80-bit
one); the SVD anchor; the objective never rises and the lab half-sweep leaves no gradient; transform, state, inactive
labs, pass-through, the stopping rule; every refusal; the binding of libmmgnn_mf.so from its header and the refusals of
its C ABI; the baseline plumbing on a small synthetic graph through the numpy path."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib, ops
from mmgnn import evaluate as ev
from mmgnn import lowrank as lr
from mmgnn.lowrank import LowRankLabImputer
from mmgnn.synth import make_graph
from mmgnn.train import EdgeMasker
import mf_ref as ref

F32 = np.float32
LENGTHS = (0, 1, 2, 255, 256, 257, 589, 0, 33)


# ---------------------------------------------------------------------------------- the pieces against the loops
@pytest.mark.parametrize("r", [1, 3, 8, 17])
def test_the_normal_equations_against_fsum(r):
    """Lattice inputs EQUAL the loop reference; generic ones sit inside (len + 8) 2^-53 x the absolute sum."""
    for lattice in (True, False):
        ptr, idx, y, F = ref.make_segments(LENGTHS, 50, r, seed=r, lattice=lattice)
        A, b = lr.host_normal(ptr, idx, y, F, 0.5)
        wA, wb, Aa, ba = ref.normal(ptr, idx, y, F, 0.5)
        assert np.array_equal(A, A.transpose(0, 2, 1)), "exactly symmetric"
        if lattice:
            assert np.array_equal(A, wA) and np.array_equal(b, wb)
        else:
            n = np.diff(ptr)
            assert np.all(np.abs(A - wA) <= ref.sum_bound(n[:, None, None], Aa))
            assert np.all(np.abs(b - wb) <= ref.sum_bound(n[:, None], ba))
        empty = np.diff(ptr) == 0
        assert np.array_equal(A[empty], np.broadcast_to(0.5 * np.eye(r), (int(empty.sum()), r, r))) and not b[empty].any()


@pytest.mark.parametrize("r", [1, 2, 8, 32])
def test_the_solve_is_inside_its_stated_rounding_and_counts_bad_pivots(r):
    ptr, idx, y, F = ref.make_segments(LENGTHS, 50, r, seed=10 + r)
    A, b = lr.host_normal(ptr, idx, y, F, 1.0)
    x, bad = lr.host_solve(A, b)
    assert bad == 0
    for s in range(len(ptr) - 1):
        want = ref.solve_ld(A[s], b[s])
        resid = np.abs(A[s] @ x[s] - b[s]).max()
        assert resid <= 8 * r * r * ref.U * np.abs(A[s]).sum(1).max() * max(np.abs(x[s]).max(), 1e-300), s
        # the forward error of a backward-stable solve: the residual bound times the condition number
        cond = np.linalg.cond(A[s])
        assert np.abs(x[s].astype(ref.LD) - want).max() <= 8 * r * r * ref.U * cond * max(np.abs(x[s]).max(), 1e-300), s
    half, bad2 = lr.host_half_sweep(ptr, idx, y, F, 1.0)
    keep = np.diff(ptr) > 0
    assert bad2 == 0 and np.array_equal(half[keep], x[keep]) and not half[~keep].any(), "an empty segment: the zero vector"
    Abad = np.stack([-5.0 * np.eye(4), np.eye(4)])
    _, bad = lr.host_solve(Abad, np.ones((2, 4)))
    assert bad == 4, "four pivots of -5; the identity has none"


def test_the_index_is_numpys_stable_sorts():
    p, lab, v = ref.make_triples(70, 9, 0.4, seed=3, empty_lab=4)
    ix = lr.host_index(p, lab, v, 70, 9)
    key = p * 9 + lab
    op, ol = np.argsort(key, kind="stable"), np.argsort(lab * 70 + p, kind="stable")
    assert np.array_equal(ix["p_idx"], lab[op]) and np.array_equal(ix["p_val"], v[op]) and np.array_equal(ix["l_idx"], p[ol])
    assert np.array_equal(ix["p_ptr"], np.searchsorted(p[op], np.arange(71))) and ix["p_ptr"][-1] == p.size
    assert np.array_equal(ix["l_ptr"], np.searchsorted(lab[ol], np.arange(10)))
    assert ix["count"][4] == 0 and ix["center"][4] == 0.0 and ix["count"].sum() == p.size
    for l in range(9):
        if ix["count"][l]:
            assert abs(ix["center"][l] - float(v[lab == l].astype(ref.LD).mean())) <= 4 * ref.U * np.abs(v[lab == l]).max()
    assert np.array_equal(ix["p_y"], v[op].astype(np.float64) - ix["center"][lab[op]])
    assert np.array_equal(ix["l_y"], v[ol].astype(np.float64) - ix["center"][lab[ol]])


# ---------------------------------------------------------------------------------- the anchors
def svd_matrix():
    rng = np.random.default_rng(7)
    Q1, _ = np.linalg.qr(rng.standard_normal((40, 12)))
    Q2, _ = np.linalg.qr(rng.standard_normal((12, 12)))
    sv = np.array([8, 4, 2, 1, 0.5, 0.25] + [0.1] * 6)
    return ((Q1 * sv) @ Q2.T).astype(F32)


def test_a_fully_observed_matrix_gives_the_soft_thresholded_svd():
    """40 x 12, singular values 8, 4, 2, 1, .5, .25 and .1 six times; centre forced to zero, rank 3, reg 0.5, 200 rounds:
    U V^T is the rank-3 SVD with its singular values reduced by reg, within 1e-12 of the largest entry."""
    X = svd_matrix()
    imp = LowRankLabImputer(rank=3, reg=0.5, tol=0, max_iter=200).fit_matrix(X, center=np.zeros(12))
    u, s, vt = np.linalg.svd(X.astype(np.float64), full_matrices=False)
    want = (u[:, :3] * (s[:3] - 0.5)) @ vt[:3]
    got = imp.patient_factors_ @ imp.lab_factors_.T
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"SVD anchor after 200 rounds: {err:.2e} of the largest entry")
    assert imp.n_iter_ == 200 and err <= 1e-12


@functools.lru_cache(maxsize=None)
def sparse_case():
    p, lab, v = ref.make_triples(300, 20, 0.3, seed=11)
    return p, lab, v, lr.host_index(p, lab, v, 300, 20)


def test_the_objective_never_rises_and_the_lab_half_sweep_leaves_no_gradient():
    """300 x 20, 30 % observed, rank 4, reg 1, 30 rounds: F falls (to 1e-12 relative) at every half-sweep; directly
    after a lab half-sweep the gradient of F with respect to V is below 1e-10 max|b|."""
    p, lab, v, ix = sparse_case()
    V = np.random.default_rng(0).standard_normal((20, 4)) * 0.1
    U = np.zeros((300, 4))
    F = lambda: lr._objective_value(lr.host_objective(ix, U, V), 1.0)                   # noqa: E731
    prev, worst_rise, worst_grad = F(), 0.0, 0.0
    for _ in range(30):
        U, _ = lr.host_half_sweep(ix["p_ptr"], ix["p_idx"], ix["p_y"], V, 1.0)
        now = F()
        worst_rise, prev = max(worst_rise, (now - prev) / prev), now
        V, _ = lr.host_half_sweep(ix["l_ptr"], ix["l_idx"], ix["l_y"], U, 1.0)
        now = F()
        worst_rise, prev = max(worst_rise, (now - prev) / prev), now
        A, b = lr.host_normal(ix["l_ptr"], ix["l_idx"], ix["l_y"], U, 1.0)
        grad = np.einsum("skl,sl->sk", A, V) - b                                       # half the gradient of F in V
        worst_grad = max(worst_grad, float(np.abs(grad).max() / np.abs(b).max()))
    print(f"largest relative rise of F over 60 half-sweeps {worst_rise:.2e}; gradient after a lab half-sweep "
          f"{worst_grad:.2e} of max|b|")
    assert worst_rise <= 1e-12 and worst_grad <= 1e-10


@pytest.mark.parametrize("n, L, rank", [(60, 7, 2), (257, 17, 4)])
def test_the_restatement_against_the_80_bit_chain(n, L, rank):
    """Three rounds: factors and objective within the rounding of a few hundred float64 operations of the 80-bit chain
    (1e-9 relative: conditioning included, far above what was seen, far below any mistake in the algorithm)."""
    p, lab, v = ref.make_triples(n, L, 0.3, seed=n + L, empty_lab=2)
    imp = LowRankLabImputer(rank=rank, reg=1.0, tol=0, max_iter=3, seed=5).fit(p, lab, v, n, L)
    V0 = np.random.default_rng(5).standard_normal((L, rank)) * 0.1
    Uw, Vw, hist, center = ref.als(p, lab, v, n, L, V0, 1.0, 3)
    dU = float(np.abs(imp.patient_factors_.astype(ref.LD) - Uw).max())
    dV = float(np.abs(imp.lab_factors_.astype(ref.LD) - Vw).max())
    print(f"({n}, {L}) rank {rank}: U {dU:.2e}, V {dV:.2e} from the 80-bit chain")
    assert max(dU, dV) <= 1e-9 * float(np.abs(Uw).max())
    assert np.allclose(imp.history_, hist, rtol=1e-9, atol=0) and imp.n_iter_ == 3
    assert not imp.lab_factors_[2].any() and np.isnan(imp.impute_matrix()[:, 2]).all()


# ---------------------------------------------------------------------------------- the imputer
@functools.lru_cache(maxsize=None)
def fitted(tol=0.0):
    p, lab, v = ref.make_triples(120, 9, 0.4, seed=21, empty_lab=6)
    return p, lab, v, LowRankLabImputer(rank=3, reg=0.7, tol=tol, max_iter=12).fit(p, lab, v, 120, 9)


def test_transform_of_the_training_triples_equals_the_stored_patient_factors():
    p, lab, v, imp = fitted()
    out = imp.impute_matrix()
    again = imp.transform(p, lab, v, 120)
    assert out.dtype == F32 and out.shape == (120, 9)
    assert np.array_equal(again.view(np.int32), out.view(np.int32)), "the closing half-sweep: U is the fold-in of V"
    st = imp._state
    recon = lr.host_predict(np.repeat(np.arange(120), 9), np.tile(np.arange(9), 120), imp.patient_factors_, st["V"],
                            st["center"], st["count"], -np.inf, np.inf).reshape(120, 9)
    miss = np.ones((120, 9), bool)
    miss[p, lab] = False
    assert np.array_equal(out[miss].view(np.int32), recon[miss].view(np.int32))
    rows = np.array([5, 119, 0, 77])
    assert np.array_equal(imp.impute_matrix(rows).view(np.int32), out[rows].view(np.int32))
    cols = np.array([0, 8, 3, 6])
    assert np.array_equal(imp.predict(rows, cols).view(np.int32), recon[rows, cols].view(np.int32))
    sel = np.isin(p, [3, 50])                                         # two new patients: rows are independent
    two = imp.transform(np.where(p[sel] == 3, 0, 1), lab[sel], v[sel], 2)
    assert np.array_equal(two.view(np.int32), out[[3, 50]].view(np.int32))
    t = imp.transform(torch.from_numpy(p), torch.from_numpy(lab), torch.from_numpy(v), 120)
    assert torch.is_tensor(t) and np.array_equal(t.numpy().view(np.int32), out.view(np.int32))


def test_an_inactive_lab_is_nan_and_observed_cells_pass_through_bit_for_bit():
    p, lab, v, imp = fitted()
    out = imp.impute_matrix()
    assert np.isnan(out[:, 6]).all() and not np.isnan(np.delete(out, 6, axis=1)).any()
    assert np.isnan(imp.predict(np.array([0, 1]), np.array([6, 6]))).all()
    assert not imp.lab_factors_[6].any() and imp._state["count"][6] == 0
    assert np.array_equal(out[p, lab].view(np.int32), v.view(np.int32))
    odd = v.copy()
    odd[0] = F32(-0.0)
    o2 = LowRankLabImputer(rank=2, max_iter=2).fit(p, lab, odd, 120, 9).impute_matrix()
    assert np.array_equal(o2[p, lab].view(np.int32), odd.view(np.int32)), "the sign of a zero included"
    clipped = LowRankLabImputer(rank=3, reg=0.7, tol=0, max_iter=12, min_value=-0.25, max_value=0.5).fit(p, lab, v, 120, 9)
    c = clipped.impute_matrix()
    miss = np.ones((120, 9), bool)
    miss[p, lab] = False
    miss[:, 6] = False
    assert np.all(c[miss] >= F32(-0.25)) and np.all(c[miss] <= F32(0.5)) and (c[miss] == F32(0.5)).any()
    assert np.array_equal(c[p, lab], v), "an observed cell is never clipped"
    assert np.array_equal(c[miss], np.clip(out[miss], F32(-0.25), F32(0.5)))


def test_fit_matrix_and_the_stopping_rule():
    p, lab, v, full = fitted()
    X = np.full((120, 9), np.nan, F32)
    X[p, lab] = v
    m = LowRankLabImputer(rank=3, reg=0.7, tol=0, max_iter=12).fit_matrix(X)
    assert np.array_equal(m.impute_matrix().view(np.int32), full.impute_matrix().view(np.int32))
    tm = LowRankLabImputer(rank=3, reg=0.7, tol=0, max_iter=2).fit_matrix(torch.from_numpy(X))
    assert torch.is_tensor(tm.impute_matrix()) and torch.is_tensor(tm.patient_factors_)
    h = full.history_
    assert full.n_iter_ == 12 and len(h) == 12 and all(b <= a for a, b in zip(h, h[1:]))
    rel = [(h[i - 1] - h[i]) / h[i - 1] for i in range(1, 12)]
    k = next(i for i in range(1, 11) if rel[i] < rel[i - 1] / 1.5 and all(x > rel[i] * 1.2 for x in rel[:i]))
    tol = float(np.sqrt(rel[k] * min(rel[:k])))
    assert min(rel[:k]) > 1.2 * tol and rel[k] < tol / 1.2, "an asserted gap: rounding cannot cross it"
    imp = LowRankLabImputer(rank=3, reg=0.7, tol=tol, max_iter=12).fit(p, lab, v, 120, 9)
    assert imp.n_iter_ == k + 2 and imp.history_ == h[:k + 2], "stops after the round whose relative gain is below tol"


def test_state_dict_round_trip():
    p, lab, v, imp = fitted()
    state = imp.state_dict()
    assert all(torch.is_tensor(state[k]) for k in ("V", "center", "count"))
    assert state["V"].shape == (9, 3) and state["V"].dtype == torch.float64 and "U" not in state
    other = LowRankLabImputer().load_state_dict({k: (t.clone() if torch.is_tensor(t) else t) for k, t in state.items()})
    assert other.n_iter_ == 12 and other.history_ == imp.history_ and other.rank == 3 and other.reg == 0.7
    assert np.array_equal(other.transform(p, lab, v, 120).view(np.int32), imp.impute_matrix().view(np.int32))
    for call in (other.impute_matrix, lambda: other.predict(np.array([0]), np.array([0])), lambda: other.patient_factors_):
        with pytest.raises(RuntimeError, match="transform"):
            call()
    with pytest.raises(KeyError, match="center"):
        LowRankLabImputer().load_state_dict({k: t for k, t in state.items() if k != "center"})
    with pytest.raises(RuntimeError, match="fit"):
        LowRankLabImputer().transform(p, lab, v, 120)


def test_a_user_start_is_honoured():
    p, lab, v, _ = fitted()
    V0 = np.random.default_rng(3).standard_normal((9, 3))
    a = LowRankLabImputer(rank=3, tol=0, max_iter=2, init=V0).fit(p, lab, v, 120, 9)
    b = LowRankLabImputer(rank=3, tol=0, max_iter=2, init=torch.from_numpy(V0)).fit(p, lab, v, 120, 9)
    c = LowRankLabImputer(rank=3, tol=0, max_iter=2, seed=3).fit(p, lab, v, 120, 9)
    assert np.array_equal(a.lab_factors_, b.lab_factors_) and not np.array_equal(a.lab_factors_, c.lab_factors_)
    ix = lr.host_index(p, lab, v, 120, 9)
    V0[6] = 0.0
    U1, _ = lr.host_half_sweep(ix["p_ptr"], ix["p_idx"], ix["p_y"], V0, 1.0)
    one = LowRankLabImputer(rank=3, tol=0, max_iter=1, init=V0).fit(p, lab, v, 120, 9)
    V1, _ = lr.host_half_sweep(ix["l_ptr"], ix["l_idx"], ix["l_y"], U1, 1.0)
    assert np.array_equal(one.lab_factors_, V1)


# ---------------------------------------------------------------------------------- refusals
def test_every_refusal():
    p, lab, v = np.array([0, 0, 2]), np.array([0, 1, 1]), np.array([1.0, 2.0, 3.0], F32)
    for kw, msg in ((dict(rank=0), "rank"), (dict(rank=33), "rank"), (dict(rank=2.0), "rank"), (dict(reg=0.0), "reg"),
                    (dict(reg=-1.0), "reg"), (dict(reg=float("nan")), "reg"), (dict(reg=float("inf")), "reg"),
                    (dict(max_iter=0), "max_iter"), (dict(tol=-1e-3), "tol"), (dict(min_value=1.0, max_value=1.0), "min_value"),
                    (dict(rank=2, init=np.zeros((3, 2))), "init"), (dict(rank=2, init=np.full((2, 2), np.nan)), "init")):
        with pytest.raises(ValueError, match=msg):
            LowRankLabImputer(**kw).fit(p, lab, v, 3, 2)
    for args, msg in (((p, lab, v, 3, 2049), "n_labs"), ((p, lab, v, 3, 0), "n_labs"), ((p, lab, v, 0, 2), "n_patients"),
                      ((p, lab, v, 2, 2), "patient index"), ((p, lab, v, 3, 1), "lab index"),
                      ((p, lab, v[:2], 3, 2), "one entry per cell"), ((p.astype(np.float64), lab, v, 3, 2), "integers"),
                      ((p, lab, np.array([1, np.nan, 3], F32), 3, 2), "NaN"),
                      ((p, lab, np.array([1, np.inf, 3], F32), 3, 2), "infinite"),
                      ((np.array([0, 0, 2]), np.array([1, 1, 1]), v, 3, 2), "duplicate")):
        with pytest.raises(ValueError, match=msg):
            LowRankLabImputer().fit(*args)
    with pytest.raises(ValueError, match="2-D"):
        LowRankLabImputer().fit_matrix(np.zeros(4, F32))
    with pytest.raises(ValueError, match="center"):
        LowRankLabImputer().fit(p, lab, v, 3, 2, center=np.zeros(3))
    imp = LowRankLabImputer(rank=2, max_iter=2).fit(p, lab, v, 3, 2)
    assert isinstance(imp.impute_matrix(), np.ndarray) and imp.impute_matrix().shape == (3, 2)
    wide = LowRankLabImputer(rank=1, max_iter=1).fit(p, lab, v, 3, 2048)
    assert wide.impute_matrix().shape == (3, 2048), "the project's lab limit"
    with pytest.raises(ValueError, match="lab index"):
        imp.transform(p, np.array([0, 1, 2]), v, 3)
    with pytest.raises(ValueError, match="patient index"):
        imp.predict(np.array([3]), np.array([0]))
    with pytest.raises(ValueError, match="lab index"):
        imp.predict(np.array([0]), np.array([2]))
    with pytest.raises(ValueError, match="1 patients but 2 labs"):
        imp.predict(np.array([0]), np.array([0, 1]))
    with pytest.raises(RuntimeError, match="fit"):
        LowRankLabImputer().impute_matrix()
    from mmgnn import mf_ops
    with pytest.raises(_lib.MmgError, match="device tensor"):               # never the host path behind the kernels' door
        mf_ops.mf_index(torch.from_numpy(p), torch.from_numpy(lab), torch.from_numpy(v), 3, 2)


# ---------------------------------------------------------------------------------- the binding
def test_the_mf_header_parses_and_names_what_the_library_defines():
    from mmgnn import mf_ops as m
    b = m.BINDING
    assert isinstance(b, _lib.Binding) and b.stem == "mf"
    assert os.path.basename(b.lib_path) == "libmmgnn_mf.so" and os.path.basename(b.header_path) == "mmgnn_mf.h"
    assert (m.DEFINES, m.SIGNATURES, m.PARAMS) == (b.defines, b.signatures, b.params)
    text = re.sub(r"/\*.*?\*/", "", open(b.header_path).read(), flags=re.S)
    assert sorted(re.findall(r"^\s*#\s*define\s+(MMG_\w+)", text, flags=re.M)) == sorted(b.defines) and b.defines
    for name, v in b.defines.items():
        assert type(v) is int and getattr(m, name) == v
    assert m.MF_MAX_LABS == lr.MAX_LABS == 2048 and m.MF_MAX_RANK == lr.MAX_RANK == 32 and m.MF_CHUNK == ref.CHUNK
    assert m.MF_SPLIT % m.MF_CHUNK == 0 and m.MF_SPLIT > m.MF_CHUNK
    assert not set(b.signatures) & set(_lib.SIGNATURES)
    assert os.path.exists(b.lib_path), f"{b.lib_path} is not built (make -C multi-modal-gnn_amd/csrc)"
    ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)               # the satellite links against it
    raw = ctypes.CDLL(b.lib_path)
    for sym in b.signatures:
        assert hasattr(raw, sym), sym
    assert sorted(b.signatures) == sorted(
        f"mmg_mf_{s}" for s in ("plan", "index", "index_ws_bytes", "half_sweep", "half_sweep_ws_bytes", "objective",
                                "objective_ws_bytes", "predict_pairs", "impute_matrix"))
    with_ws = [sym for sym, params in b.params.items() if any(p[0] == "ws" for p in params)]
    assert sorted(with_ws) == ["mmg_mf_half_sweep", "mmg_mf_index", "mmg_mf_objective"]
    for sym in with_ws:
        assert sym + "_ws_bytes" in b.signatures and b.signatures[sym + "_ws_bytes"][0] is ctypes.c_size_t, sym
        assert [p[0] for p in b.params[sym]][-3:] == ["ws", "ws_bytes", "stream"], sym
        assert b.params[sym][-3][1:] == ("void", 1) and b.params[sym][-2][1:] == ("size_t", 0), sym
    for sym, params in b.params.items():
        if not sym.endswith(("_plan", "_ws_bytes")):
            assert params[-1][0] == "stream", sym
    assert sorted(ops._plans(b)) == sorted(b.signatures)
    makefile = open(os.path.join(os.path.dirname(b.lib_path), "csrc", "Makefile")).read()
    assert re.search(r"^SATELLITES = .*\bmf\b", makefile, flags=re.M)


def test_the_plan_and_the_host_refusals_of_the_library():
    """mmg_mf_plan and every argument check run on the host: no device is needed (null device pointers are refused
    after the shape)."""
    from mmgnn import mf_ops as m
    lib = m.load()
    CH, SPLIT = m.MF_CHUNK, m.MF_SPLIT
    for n, want in ((0, m.MMG_MF_PATH_EMPTY), (1, m.MMG_MF_PATH_WAVE), (CH, m.MMG_MF_PATH_WAVE), (CH + 1, m.MMG_MF_PATH_WAVE),
                    (SPLIT, m.MMG_MF_PATH_WAVE), (SPLIT + 1, m.MMG_MF_PATH_SPLIT), (10 ** 6, m.MMG_MF_PATH_SPLIT)):
        assert m.mf_plan(n) == (want, -(-n // CH))
    for n in (-1, 2 ** 31 - 1):
        with pytest.raises(_lib.MmgError, match="mf_plan"):
            m.mf_plan(n)
    err = lambda: _lib.load().mmg_last_error()                                          # noqa: E731
    E_ARG, E_WS = _lib.MMG_E_ARG, _lib.MMG_E_WS
    # the workspace sizes: 0 for an unsupported shape, else at least what the plan needs
    assert lib.mmg_mf_half_sweep_ws_bytes(10, 5000, 4) >= (5000 * 9 // (8 * CH)) * 14 * 8 + 11 * 4
    for seg, nnz, r in ((0, 5, 4), (10, -1, 4), (10, 5, 0), (10, 5, 33), (2 ** 31 - 1, 5, 4), (10, 2 ** 31 - 1, 4)):
        assert lib.mmg_mf_half_sweep_ws_bytes(seg, nnz, r) == 0
    assert lib.mmg_mf_index_ws_bytes(100, 10, 5) > 100 * 36
    for nnz, P, L in ((-1, 10, 5), (5, 0, 5), (5, 10, 0), (5, 10, 2049), (2 ** 31 - 1, 10, 5), (5, 2 ** 31 - 1, 5)):
        assert lib.mmg_mf_index_ws_bytes(nnz, P, L) == 0 and lib.mmg_mf_objective_ws_bytes(nnz, P, L, 4) == 0
    assert lib.mmg_mf_objective_ws_bytes(5, 10, 5, 0) == 0 and lib.mmg_mf_objective_ws_bytes(5, 10, 5, 33) == 0
    assert lib.mmg_mf_objective_ws_bytes(5, 10, 5, 32) > 0

    def sweep(seg=10, nnz=5, m_=7, r=4, reg=1.0):
        return lib.mmg_mf_half_sweep(None, None, None, seg, nnz, None, m_, r, reg, None, None, None, None, 0, None)

    for kw, msg in ((dict(r=0), b"rank 0"), (dict(r=33), b"rank 33"), (dict(reg=0.0), b"reg"), (dict(reg=-1.0), b"reg"),
                    (dict(reg=float("inf")), b"reg"), (dict(reg=float("nan")), b"reg"), (dict(seg=0), b"segments"),
                    (dict(nnz=-1), b"pairs"), (dict(m_=0), b"other side"), (dict(), b"null pointer")):
        assert sweep(**kw) == E_ARG and msg in err(), kw

    def index(nnz=5, P=10, L=5):
        return lib.mmg_mf_index(None, None, None, nnz, P, L, None, None, None, None, None, None, None, None, None, None,
                                None, 0, None)

    for kw, msg in ((dict(L=0), b"0 labs"), (dict(L=2049), b"2049 labs"), (dict(P=0), b"patients"), (dict(nnz=-1), b"pairs"),
                    (dict(), b"null pointer")):
        assert index(**kw) == E_ARG and msg in err(), kw
    assert lib.mmg_mf_objective(None, None, None, 5, 10, 0, None, None, 4, None, None, 0, None) == E_ARG and b"labs" in err()
    assert lib.mmg_mf_objective(None, None, None, 5, 10, 5, None, None, 33, None, None, 0, None) == E_ARG and b"rank" in err()
    assert lib.mmg_mf_objective(None, None, None, 5, 10, 5, None, None, 4, None, None, 0, None) == E_ARG
    assert b"null pointer" in err()

    def predict(L=5, r=4, lo=-1.0, hi=1.0):
        return lib.mmg_mf_predict_pairs(None, None, 5, None, 10, None, L, r, None, None, lo, hi, None, None)

    for kw, msg in ((dict(L=0), b"labs"), (dict(L=2049), b"labs"), (dict(r=0), b"rank"), (dict(r=33), b"rank"),
                    (dict(lo=1.0, hi=1.0), b"clip"), (dict(lo=float("nan")), b"clip"), (dict(), b"null pointer")):
        assert predict(**kw) == E_ARG and msg in err(), kw

    def impute(L=5, r=4, ld=5, lo=-1.0, hi=1.0):
        return lib.mmg_mf_impute_matrix(None, 3, None, 10, None, L, r, None, None, lo, hi, None, None, None, 5, None, ld, None)

    for kw, msg in ((dict(L=0), b"labs"), (dict(L=2049, ld=4000), b"labs"), (dict(r=0), b"rank"), (dict(r=33), b"rank"),
                    (dict(ld=4), b"ld_out"), (dict(lo=2.0), b"clip"), (dict(), b"null pointer")):
        assert impute(**kw) == E_ARG and msg in err(), kw
    assert E_ARG != E_WS


# ---------------------------------------------------------------------------------- the drivers
def test_the_baseline_plumbing_on_a_synthetic_graph_through_the_numpy_path():
    g = make_graph(1, seed=0)
    masker = EdgeMasker(g)
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    assert "low_rank" in ev.BASELINES and ev.BASELINES[:4] == ("global_mean", "per_lab_mean", "nearest_neighbor",
                                                               "chained_equations")
    tr_ei, tr_v, _, _ = masker.get_masked_data("train", want_mask=False)
    te_ei, te_v, _, _ = masker.get_masked_data("test", want_mask=False)
    fitted_ = ev.fit_baselines(("per_lab_mean", "low_rank"), tr_ei, tr_v.reshape(-1), L, P)
    kind, (imp, g_mean) = fitted_["low_rank"]
    assert kind == "low_rank" and isinstance(imp, LowRankLabImputer) and 1 <= imp.n_iter_ <= 20 and imp.rank == 8
    pairs = ev.baseline_pairs(fitted_["low_rank"], te_ei[0], te_ei[1])
    assert torch.is_tensor(pairs) and pairs.dtype == torch.float32 and pairs.shape == (te_ei.shape[1],)
    assert bool(torch.isfinite(pairs).all())
    rows = torch.tensor([0, 5, P - 1])
    dense = ev.baseline_matrix(fitted_["low_rank"], rows, L)
    assert dense.shape == (3, L) and bool(torch.isfinite(dense).all())
    X = imp.impute_matrix()
    assert torch.equal(dense, torch.where(torch.isnan(X[rows]), g_mean, X[rows]))
    tr = tr_ei.numpy()
    assert np.array_equal(X[tr[0], tr[1]].numpy(), tr_v.reshape(-1).numpy()), "train values pass through"
    assert torch.equal(pairs, X[te_ei[0], te_ei[1]]), "a test pair is no train pair: the matrix holds its reconstruction"
    res = ev.evaluate_lowrank_baseline(g, masker, "test", rank=4, max_iter=3, tol=0.0)
    assert list(res) == ["low_rank"]
    want = ev.compute_regression_metrics(LowRankLabImputer(rank=4, max_iter=3, tol=0.0).fit(
        tr[0], tr[1], tr_v.reshape(-1).numpy(), P, L).predict(te_ei[0].numpy(), te_ei[1].numpy()), te_v.reshape(-1).numpy())
    assert res["low_rank"] == want and set(want) >= {"mae", "rmse", "r2"}
    print(f"synthetic x1, test split: low_rank MAE {want['mae']:.4f}")
    sweep = ev.lowrank_sweep(g, masker, ranks=(2, 4), regs=(1.0, 3.0), split="val", max_iter=3, tol=0.0)
    assert list(sweep.columns) == ["rank", "reg", "n_iter", "mae", "rmse", "r2"] and len(sweep) == 4
    assert sweep["rank"].tolist() == [2, 2, 4, 4] and sweep["reg"].tolist() == [1.0, 3.0, 1.0, 3.0]
    assert (sweep["n_iter"] == 3).all() and np.isfinite(sweep[["mae", "rmse", "r2"]].to_numpy()).all()
    va = ev.evaluate_lowrank_baseline(g, masker, "val", rank=4, reg=1.0, max_iter=3, tol=0.0)["low_rank"]
    assert sweep.iloc[2]["mae"] == va["mae"]
    with pytest.raises(ValueError, match="unknown baseline"):
        ev.fit_baselines(("median",), tr_ei, tr_v.reshape(-1), L, P)
