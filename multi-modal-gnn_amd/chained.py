"""Lab imputation by chained equations (MICE): every lab in turn is regressed on all the others, round after round,
with the semantics of ``sklearn.impute.IterativeImputer(estimator=Ridge(alpha), max_iter, tol, imputation_order,
skip_complete=False, min_value, max_value)`` over the dense patient x lab matrix of observed values (NaN = not
observed).  It is the comparator clinical imputation papers report beside the mean and nearest-neighbour baselines, and
the linear lab-to-lab structure that ``mmgnn.association`` only describes.

Definitions (this module's numpy functions are the definition; ``tests/chain_ref.py`` restates them in loops and 80-bit
arithmetic):

* ``count`` and ``center`` are the observed count and the fp64 mean of the observed values of every lab
  (``assoc_ops.assoc_colstats`` on the device, ``association.host_colstats`` here).  A lab with ``count == 0`` is
  INACTIVE: never a target, never a predictor, and its column comes back NaN -- ``KNNLabImputer``'s behaviour; sklearn
  drops such a column instead.
* the working matrix ``W`` (fp64) holds ``X`` where observed and ``center`` elsewhere.
* the targets are visited in ``imputation_order``: "ascending" (fewest missing first, ``np.argsort(missing,
  kind="mergesort")``, sklearn's default), "descending" (that order reversed), "roman" (left to right) or "arabic".
* one step for target ``j`` over ``S_j``, the rows that have lab ``j`` (every active lab, complete ones included):
  ``host_moments`` -> ``host_solve`` -> ``host_apply``.  With ``u = W - center``: ``s_a = sum u_ia``, ``G_ab = sum u_ia
  u_ib`` over ``S_j``; ``C = G - s s^T / n_j``; ``(C[P, P] + alpha I) w = C[P, j]`` over the predictors ``P`` (the
  active labs but ``j``) by the package's one Cholesky solve (``cholesky.host_cholesky_solve``), no fused multiply-add;
  ``mu = s / n_j``; every row outside ``S_j`` gets ``W_ij = clip((center_j + mu_j) + sum_a w_a ((W_ia - center_a) -
  mu_a), lo_j, hi_j)``, the sum over ``P`` ascending from 0.
* a round is one step per active lab; ``delta`` is the largest ``|new - old|`` of the round.  The fit stops after the
  round with ``delta < tol * max|X_observed|`` (sklearn's rule) or after ``max_iter`` rounds; ``tol = 0`` never stops
  early.  ``transform`` replays every stored step on new rows.
* the result is fp32, one rounding at the end; observed cells pass through bit for bit.

HIP tensors run the kernels of libmmgnn_chain.so (csrc/chain.hip): the moments on ``v_mfma_f64_16x16x4_f64`` in an order
fixed by (n, L) alone, the solve in one workgroup, the apply one thread per row; the host reads 16 bytes per round, or
nothing until the end with ``tol = 0``.  numpy arrays (and CPU tensors) run the float64 restatement of this module, which
is the checker and never a silent substitute for the kernels.  Ridge only: no ``BayesianRidge``, no posterior sampling,
no ``n_nearest_features``, no random order; at most 128 labs.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .analysis import _is_dev
from .cholesky import host_cholesky_solve

MAX_LABS = 128                        # MMG_CH_MAX_LABS
ORDERS = ("ascending", "descending", "roman", "arabic")


# ============================================================================ the numpy restatement
def visit_order(count, n: int, imputation_order: str = "ascending") -> np.ndarray:
    """The active labs (count > 0) in the order a round visits them."""
    count = np.asarray(count, np.int64)
    if imputation_order == "roman":
        order = np.arange(count.size)
    elif imputation_order == "arabic":
        order = np.arange(count.size)[::-1]
    elif imputation_order == "ascending":
        order = np.argsort((int(n) - count) / float(n), kind="mergesort")
    elif imputation_order == "descending":
        order = np.argsort((int(n) - count) / float(n), kind="mergesort")[::-1]
    else:
        raise ValueError(f"imputation_order must be one of {ORDERS}, got {imputation_order!r}")
    return np.ascontiguousarray(order[count[order] > 0], np.int64)


def predictors(count, j: int) -> np.ndarray:
    count = np.asarray(count)
    return np.array([a for a in range(count.size) if a != j and count[a] > 0], np.int64)


def host_init(X, center) -> np.ndarray:
    X = np.asarray(X, np.float32)
    return np.where(np.isfinite(X), X.astype(np.float64), np.asarray(center, np.float64)[None, :])


def host_moments(W, X, j: int, center):
    """-> (n_j, s fp64 [L], G fp64 [L, L]) of u = W - center over the rows that have lab j."""
    rows = np.isfinite(np.asarray(X)[:, j])
    u = W[rows] - np.asarray(center, np.float64)[None, :]
    G = u.T @ u
    G = np.triu(G) + np.triu(G, 1).T                                   # exactly symmetric whatever the BLAS does
    return int(rows.sum()), u.sum(0), G


def host_solve(G, s, n_j, count, j: int, alpha: float):
    """The arithmetic of mmg_chain_solve, operation by operation -> (w fp64 [L], mu fp64 [L], pivots not > 0): the
    ridge system over the predictors, then ``host_cholesky_solve``."""
    G, s = np.asarray(G, np.float64), np.asarray(s, np.float64)
    P = predictors(count, j)
    m = P.size
    nj = np.float64(int(n_j))
    with np.errstate(all="ignore"):
        C = G - (s[:, None] * s[None, :]) / nj
        A = C[np.ix_(P, P)].copy()
        A[np.arange(m), np.arange(m)] = A[np.arange(m), np.arange(m)] + np.float64(alpha)
        y, bad = host_cholesky_solve(A[None], C[P, j][None])
        w = np.zeros(s.size)
        w[P] = y[0]
        mu = s / nj
    return w, mu, bad


def host_apply(W, X, j: int, count, center, w, mu, lo, hi) -> float:
    """Rewrite column j of W on the rows without lab j (the arithmetic of mmg_chain_apply) -> the largest |new - old|."""
    rows = ~np.isfinite(np.asarray(X)[:, j])
    if not rows.any():
        return 0.0
    t = np.zeros(int(rows.sum()))
    for a in predictors(count, j):
        t = t + w[a] * ((W[rows, a] - center[a]) - mu[a])
    v = (center[j] + mu[j]) + t
    v = np.minimum(np.maximum(v, lo[j]), hi[j])
    delta = float(np.abs(v - W[rows, j]).max())
    W[rows, j] = v
    return delta


def host_finish(W, X, count) -> np.ndarray:
    X = np.asarray(X, np.float32)
    obs = np.isfinite(X)
    out = np.where(obs, X, W.astype(np.float32))
    out[~obs & (np.asarray(count) == 0)[None, :]] = np.float32(np.nan)
    return out


def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _clip_vector(v, L: int, name: str) -> np.ndarray:
    v = np.asarray(_np(v), np.float64)
    if v.ndim == 0:
        v = np.full(L, float(v))
    if v.shape != (L,):
        raise ValueError(f"{name} must be a scalar or hold one value per lab ({L}), got shape {list(v.shape)}")
    if np.isnan(v).any():
        raise ValueError(f"{name} holds NaN")
    return np.ascontiguousarray(v)


class _DeviceChain:
    """The device tensors of one fit and ``round(r)``: 3 calls per active lab, nothing read back, capturable."""

    def __init__(self, X, count, center, order, alpha, lo, hi, max_iter):
        from . import chain_ops
        self.ops = chain_ops
        dev = X.device
        n, L = X.shape
        self.X, self.count, self.center, self.order, self.alpha = X, count, center, [int(j) for j in order], float(alpha)
        self.lo, self.hi = (torch.from_numpy(v).to(dev) for v in (lo, hi))
        self.W = chain_ops.chain_init(X, center)
        self.coef = torch.zeros(max_iter, L, 2, L, dtype=torch.float64, device=dev)
        self.stat = torch.zeros(max_iter, 2, dtype=torch.int64, device=dev)      # per round: delta's bits, bad pivots
        self.mom = (torch.empty(1, dtype=torch.int64, device=dev), torch.empty(L, dtype=torch.float64, device=dev),
                    torch.empty(L, L, dtype=torch.float64, device=dev))

    def delta(self, r: int) -> torch.Tensor:
        return self.stat[r, 0:1].view(torch.float64)

    def round(self, r: int):
        o = self.ops
        n_j, s, G = self.mom
        delta, bad = self.delta(r), self.stat[r, 1:2]
        for k, j in enumerate(self.order):
            w, mu = self.coef[r, j, 0], self.coef[r, j, 1]
            o.chain_moments(self.W, self.X, j, self.center, out=self.mom)
            o.chain_solve(G, s, n_j, self.count, j, self.alpha, w, mu, bad)
            o.chain_apply(self.W, self.X, j, self.count, self.center, w, mu, self.lo, self.hi, delta, accumulate=k > 0)

    def read(self, r0: int, r1: int):
        """-> [(delta, bad pivots)] of the rounds r0 .. r1 - 1: the one read of a round."""
        rows = self.stat[r0:r1].cpu()
        return [(float(rows[i, 0:1].view(torch.float64)), int(rows[i, 1])) for i in range(r1 - r0)]


class ChainedLabImputer:
    """``fit`` the (patient, lab, value) triples (or ``fit_matrix`` a dense matrix), then ``impute_matrix`` /
    ``predict`` / ``transform``: an observed cell is passed through; a lab nobody has stays NaN."""

    def __init__(self, alpha: float = 1.0, max_iter: int = 10, tol: float = 1e-3, imputation_order: str = "ascending",
                 min_value=-np.inf, max_value=np.inf):
        self.alpha, self.max_iter, self.tol, self.imputation_order = alpha, max_iter, tol, imputation_order
        self.min_value, self.max_value = min_value, max_value
        self.n_iter_: Optional[int] = None
        self.history_: list = []
        self._state = None            # host: count, center, order, coef, lo, hi
        self._dev = {}                # device -> the same as device tensors
        self._imputed = None
        self.imputed64_ = None        # the fp64 working matrix of the fit, before the one rounding
        self._tensor_out = False

    # ------------------------------------------------------------------ validation
    def _check_params(self):
        if not (isinstance(self.alpha, (int, float)) and np.isfinite(self.alpha) and self.alpha > 0):
            raise ValueError(f"alpha must be a positive finite number, got {self.alpha!r}")
        if not (isinstance(self.max_iter, int) and self.max_iter >= 1):
            raise ValueError(f"max_iter must be an int >= 1, got {self.max_iter!r}")
        if not (isinstance(self.tol, (int, float)) and np.isfinite(self.tol) and self.tol >= 0):
            raise ValueError(f"tol must be a finite number >= 0, got {self.tol!r}")
        if self.imputation_order not in ORDERS:
            raise ValueError(f"imputation_order must be one of {ORDERS}, got {self.imputation_order!r}")

    def _clips(self, L: int):
        lo, hi = _clip_vector(self.min_value, L, "min_value"), _clip_vector(self.max_value, L, "max_value")
        if not np.all(hi > lo):
            raise ValueError("every lab needs min_value < max_value")
        return lo, hi

    @staticmethod
    def _check_shape(n: int, L: int):
        if not 1 <= L <= MAX_LABS:
            raise ValueError(f"the matrix has {L} labs, outside [1, {MAX_LABS}]")
        if not 1 <= n < 2 ** 31:
            raise ValueError(f"the matrix has {n} patients, outside [1, 2^31)")

    # ------------------------------------------------------------------ fit
    def fit(self, patient_indices, lab_indices, values, n_patients: int, n_labs: int) -> "ChainedLabImputer":
        """The triples under the checks of ``KNNLabImputer.fit`` (``association.lab_matrix``).  HIP tensors run the
        kernels, anything else the numpy restatement."""
        from .association import lab_matrix
        self._check_params()
        if not 1 <= int(n_labs) <= MAX_LABS:
            raise ValueError(f"n_labs must be in [1, {MAX_LABS}], got {n_labs}")
        X = lab_matrix(patient_indices, lab_indices, values, n_patients, n_labs)
        if not _is_dev(X) and torch.is_tensor(values):
            X = torch.from_numpy(X)
        return self.fit_matrix(X)

    def fit_matrix(self, X) -> "ChainedLabImputer":
        self._check_params()
        self._dev = {}
        if _is_dev(X):
            return self._fit_device(X)
        self._tensor_out = torch.is_tensor(X)
        return self._fit_host(X)

    def _fit_host(self, X):
        from .association import _host_matrix, _refuse_inf, host_colstats
        X = _host_matrix(X)
        n, L = X.shape
        self._check_shape(n, L)
        lo, hi = self._clips(L)
        count, center, n_inf = host_colstats(X)
        _refuse_inf(n_inf)
        order = visit_order(count, n, self.imputation_order)
        obs = np.isfinite(X)
        threshold = float(self.tol) * (float(np.abs(X[obs]).max()) if obs.any() else 0.0)
        W = host_init(X, center)
        coef = np.zeros((self.max_iter, L, 2, L))
        self.history_, bad = [], 0
        for r in range(self.max_iter):
            delta = 0.0
            for j in order:
                n_j, s, G = host_moments(W, X, j, center)
                w, mu, b = host_solve(G, s, n_j, count, j, self.alpha)
                coef[r, j, 0], coef[r, j, 1] = w, mu
                bad += b
                delta = max(delta, host_apply(W, X, j, count, center, w, mu, lo, hi))
            self._refuse_pivots(bad, r)
            self.history_.append(delta)
            if delta < threshold:
                break
        self.n_iter_ = len(self.history_)
        self._state = dict(count=count, center=center, order=order, coef=coef[:self.n_iter_].copy(), lo=lo, hi=hi)
        self.imputed64_ = W
        out = host_finish(W, X, count)
        self._imputed = torch.from_numpy(out) if self._tensor_out else out
        return self

    def _fit_device(self, X):
        from . import assoc_ops
        from .association import _dev_matrix, _refuse_inf
        X = _dev_matrix(X)
        n, L = (int(v) for v in X.shape)
        self._check_shape(n, L)
        lo, hi = self._clips(L)
        self._tensor_out = True
        count, center, n_inf = assoc_ops.assoc_colstats(X)
        top = torch.nan_to_num(X.abs(), nan=0.0).max().reshape(1).double()
        head = torch.cat([n_inf.double(), top, count.double()]).cpu().numpy()          # the one read before the rounds
        _refuse_inf(int(head[0]))
        count_h = head[2:].astype(np.int64)
        order = visit_order(count_h, n, self.imputation_order)
        threshold = float(self.tol) * float(head[1])
        chain = _DeviceChain(X, count, center, order, self.alpha, lo, hi, self.max_iter)
        self.history_ = []
        for r in range(self.max_iter):
            chain.round(r)
            if self.tol > 0:
                (delta, bad), = chain.read(r, r + 1)
                self._refuse_pivots(bad, r)
                self.history_.append(delta)
                if delta < threshold:
                    break
        if not self.tol > 0:
            for r, (delta, bad) in enumerate(chain.read(0, self.max_iter)):
                self._refuse_pivots(bad, r)
                self.history_.append(delta)
        self.n_iter_ = len(self.history_)
        coef = chain.coef[:self.n_iter_]
        self._state = dict(count=count_h, center=center.cpu().numpy(), order=order, coef=coef.cpu().numpy(), lo=lo, hi=hi)
        self._dev[X.device] = dict(count=count, center=center, coef=coef, lo=chain.lo, hi=chain.hi)
        self.imputed64_ = chain.W
        self._imputed = chain.ops.chain_finish(chain.W, X, count)
        return self

    @staticmethod
    def _refuse_pivots(bad: int, r: int):
        if bad:
            raise FloatingPointError(f"round {r}: {bad} pivots of the ridge systems were not positive")

    # ------------------------------------------------------------------ reading the fit
    def _check_fitted(self):
        if self._state is None:
            raise RuntimeError("ChainedLabImputer: call fit() first")

    def _index(self, t, what: str, hi: int):
        name = f"{what}_indices"
        if self._tensor_out:
            t = torch.as_tensor(t)
            if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f"{name} must be a 1-D integer tensor")
            t = t.to(self._imputed.device).to(torch.int64)
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= hi):
                raise ValueError(f"{what} index outside [0, {hi})")
            return t
        t = _np(t)
        if t.ndim != 1 or t.dtype.kind not in "iu":
            raise ValueError(f"{name} must be a 1-D integer array")
        if t.size and (int(t.min()) < 0 or int(t.max()) >= hi):
            raise ValueError(f"{what} index outside [0, {hi})")
        return t.astype(np.int64)

    def impute_matrix(self, patient_indices=None):
        """-> fp32 [rows, n_labs]: every lab of every requested training patient (default: all, in order)."""
        self._check_fitted()
        if self._imputed is None:
            raise RuntimeError("ChainedLabImputer: a loaded state has no training matrix; use transform()")
        if patient_indices is None:
            return self._imputed
        return self._imputed[self._index(patient_indices, "patient", self._imputed.shape[0])]

    def predict(self, patient_indices, lab_indices):
        """-> fp32 [n]: the imputed value of each (patient, lab) cell of the training matrix."""
        self._check_fitted()
        if self._imputed is None:
            raise RuntimeError("ChainedLabImputer: a loaded state has no training matrix; use transform()")
        p = self._index(patient_indices, "patient", self._imputed.shape[0])
        lab = self._index(lab_indices, "lab", self._imputed.shape[1])
        if len(p) != len(lab):
            raise ValueError(f"{len(p)} patients but {len(lab)} labs")
        return self._imputed[p, lab]

    def transform(self, X_new, return_float64: bool = False):
        """Impute new rows [rows, n_labs] with the stored steps of the fit, in order.  A HIP tensor runs the kernels."""
        self._check_fitted()
        st = self._state
        L = st["count"].size
        if _is_dev(X_new):
            from . import chain_ops
            from .association import _dev_matrix
            X = _dev_matrix(X_new)
            self._check_shape(int(X.shape[0]), int(X.shape[1]))
            if X.shape[1] != L:
                raise ValueError(f"X_new has {X.shape[1]} labs, the fit {L}")
            if bool(torch.isinf(X).any()):
                raise ValueError("X_new holds infinite cells: a lab value is finite, and NaN marks a missing one")
            d = self._device_state(X.device)
            W = chain_ops.chain_init(X, d["center"])
            scratch = torch.empty(1, dtype=torch.float64, device=X.device)
            for r in range(self.n_iter_):
                for j in st["order"]:
                    j = int(j)
                    chain_ops.chain_apply(W, X, j, d["count"], d["center"], d["coef"][r, j, 0], d["coef"][r, j, 1], d["lo"],
                                          d["hi"], scratch)
            return W if return_float64 else chain_ops.chain_finish(W, X, d["count"])
        from .association import _host_matrix
        X = _host_matrix(X_new)
        self._check_shape(*X.shape)
        if X.shape[1] != L:
            raise ValueError(f"X_new has {X.shape[1]} labs, the fit {L}")
        if np.isinf(X).any():
            raise ValueError("X_new holds infinite cells: a lab value is finite, and NaN marks a missing one")
        W = host_init(X, st["center"])
        for r in range(self.n_iter_):
            for j in st["order"]:
                host_apply(W, X, int(j), st["count"], st["center"], st["coef"][r, j, 0], st["coef"][r, j, 1], st["lo"],
                           st["hi"])
        out = W if return_float64 else host_finish(W, X, st["count"])
        return torch.from_numpy(out) if torch.is_tensor(X_new) else out

    def _device_state(self, device):
        if device not in self._dev:
            st = self._state
            self._dev[device] = {k: torch.from_numpy(np.ascontiguousarray(st[k])).to(device)
                                 for k in ("count", "center", "coef", "lo", "hi")}
        return self._dev[device]

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        """Everything ``transform`` needs, as CPU tensors and plain values: no training matrix."""
        self._check_fitted()
        st = self._state
        out = {k: torch.from_numpy(np.array(st[k])) for k in ("count", "center", "order", "coef", "lo", "hi")}
        out.update(alpha=float(self.alpha), max_iter=int(self.max_iter), tol=float(self.tol),
                   imputation_order=self.imputation_order, n_iter=int(self.n_iter_), history=list(self.history_))
        return out

    def load_state_dict(self, state: dict) -> "ChainedLabImputer":
        need = ("count", "center", "order", "coef", "lo", "hi", "alpha", "max_iter", "tol", "imputation_order", "n_iter",
                "history")
        missing = [k for k in need if k not in state]
        if missing:
            raise KeyError(f"ChainedLabImputer.load_state_dict: missing {missing}")
        st = dict(count=_np(state["count"]).astype(np.int64), center=_np(state["center"]).astype(np.float64),
                  order=_np(state["order"]).astype(np.int64), coef=_np(state["coef"]).astype(np.float64),
                  lo=_np(state["lo"]).astype(np.float64), hi=_np(state["hi"]).astype(np.float64))
        L, n_iter = st["count"].size, int(state["n_iter"])
        if st["coef"].shape != (n_iter, L, 2, L) or st["center"].shape != (L,) or st["lo"].shape != (L,) \
                or st["hi"].shape != (L,) or not 1 <= L <= MAX_LABS:
            raise ValueError("ChainedLabImputer.load_state_dict: inconsistent shapes")
        self.alpha, self.max_iter, self.tol = float(state["alpha"]), int(state["max_iter"]), float(state["tol"])
        self.imputation_order = state["imputation_order"]
        self.min_value, self.max_value = st["lo"].copy(), st["hi"].copy()
        self.n_iter_, self.history_ = n_iter, list(state["history"])
        self._state, self._dev, self._imputed, self.imputed64_ = st, {}, None, None
        return self
