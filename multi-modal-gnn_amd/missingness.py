"""Per-lab measurement propensity: P(lab j is measured | what is known about the patient), one L2-penalised logistic
regression per lab over the same patients, with the minimiser of ``sklearn.linear_model.LogisticRegression(C=C,
penalty="l2", fit_intercept=True)``.  Every error the project reports is an average over MEASURED cells; what it ships
are values for cells that were not.  A model of which cells get measured is what an inverse-probability-weighted error,
a classifier two-sample test or a weighted conformal quantile start from.

Definitions (this module's numpy functions are the definition; ``tests/prop_ref.py`` restates them in loops and 80-bit
arithmetic; ``include/mmgnn_prop.h`` spells out every order):

* the features ``x`` are dense and finite, ``1 <= D <= 128``; ``u = x - mean`` with ``mean`` the fp64 column means
  (``assoc_ops.assoc_colstats`` on the device, ``association.host_colstats`` here).  The intercept is not penalised, so
  centring moves only the intercept; ``intercept_`` is reported for the UNCENTRED ``x``.
* a lab that nobody or everybody has is DEGENERATE: coefficients 0, ``n_iter_`` 0, intercept ``-inf`` / ``+inf``, the
  propensity exactly 0 / 1.
* Newton's method from ``w = 0, b = logit(mean y_j)``: one round is ``host_link`` (z, p, q, s = p q, r = p - y, the
  loss) -> ``host_moments`` (H = U~^T S U~, g = U~^T r) -> ``host_solve`` (H + diag(1/C, .., 1/C, 0), right-looking
  Cholesky, the decrement g~ . H~^-1 g~) -> ``host_update``: when the decrement at the trial point is at most ``tol * n``
  the lab has converged (tested FIRST: at the last step F moves by rounding only) and the Newton step from there is taken
  as the result without another evaluation; else the trial point is accepted when F did not rise; otherwise the step is
  halved.  ``n_iter_`` counts the trial points after the start, a halved retry included; ``max_iter`` bounds
  it.  A fit is ``max_iter + 1`` rounds; a lab that has converged is frozen.

HIP tensors run the kernels of libmmgnn_prop.so (csrc/prop.hip): every lab advances in the same launches, the weighted
Grams on ``v_mfma_f64_16x16x4_f64`` in an order fixed by (n, D) alone, a converged lab frozen by a flag on the device;
nothing is read back until the rounds are over.  numpy arrays (and CPU tensors) run the float64 restatement of this
module, which is the checker and never a silent substitute for the kernels.

``ipw_metrics`` turns the propensities into inverse-probability-weighted errors (``mmg_prop_pair_sums``).

Staying out: L1 / elastic net, class weights, multinomial targets, AUROC, more than 128 features, weighted conformal
quantiles, the classifier two-sample test as a ``shift`` option, Little's MCAR test.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import NamedTuple

import numpy as np
import pandas as pd
import torch

from .analysis import _is_dev
from .cholesky import host_cholesky_solve

MAX_FEATURES = 128                    # MMG_PR_MAX_FEATURES
MAX_LABS = 512                        # MMG_PR_MAX_LABS
LINK_ROWS = 64                        # MMG_PR_LINK_ROWS
ACTIVE, N_ITER, CONVERGED, HALVINGS, STARTED, BAD = range(6)        # MMG_PR_* of the int32 state
N_STATE, N_FSTATE = 8, 4


# ============================================================================ the numpy restatement
def host_link(X, mean, y, coef):
    """One lab: the arithmetic of mmg_prop_link, operation by operation -> (z, p, q, s, r, t), fp64 [n] each."""
    u = np.asarray(X, np.float32).astype(np.float64) - np.asarray(mean, np.float64)[None, :]
    D = u.shape[1]
    y = np.asarray(y) != 0
    with np.errstate(all="ignore"):
        z = np.full(u.shape[0], np.float64(coef[D]))
        for a in range(D):
            z = z + u[:, a] * np.float64(coef[a])
        e = np.exp(-np.abs(z))
        d = 1.0 + e
        big, small = 1.0 / d, e / d
        p, q = np.where(z >= 0.0, big, small), np.where(z >= 0.0, small, big)
        s = p * q
        r = np.where(y, -q, p)
        t = (np.where(z > 0.0, z, 0.0) - np.where(y, z, 0.0)) + np.log1p(e)
    return z, p, q, s, r, t


def host_loss_blocks(t) -> np.ndarray:
    """The loss terms of one lab -> the sums of its blocks of 64 rows, each by the tree of mmg_prop_link."""
    t = np.asarray(t, np.float64)
    blocks = (t.size + LINK_ROWS - 1) // LINK_ROWS
    v = np.zeros(blocks * LINK_ROWS)
    v[:t.size] = t
    v = v.reshape(blocks, LINK_ROWS)
    o = LINK_ROWS // 2
    while o:
        v = v[:, :o] + v[:, o:2 * o]
        o //= 2
    return v[:, 0].copy()


def serial_sum(v) -> float:
    """v_0 + v_1 + .. from 0, left to right."""
    v = np.asarray(v, np.float64)
    return float(np.cumsum(v)[-1]) if v.size else 0.0


def host_moments(X, mean, s, r):
    """-> (H fp64 [M, M], g fp64 [M]) with u~ = [x - mean, 1]: H = sum s_i u~_i u~_i^T (exactly symmetric), g = sum r_i u~_i."""
    u = np.asarray(X, np.float32).astype(np.float64) - np.asarray(mean, np.float64)[None, :]
    ut = np.concatenate([u, np.ones((u.shape[0], 1))], axis=1)
    H = (s[:, None] * ut).T @ ut
    H = np.triu(H) + np.triu(H, 1).T
    return H, ut.T @ r


def host_solve(H, g, trial, C: float):
    """The arithmetic of mmg_prop_solve, operation by operation -> (delta fp64 [M], decrement, pivots not > 0): the
    Newton system, ``host_cholesky_solve``, then the decrement in ascending order."""
    A = np.array(H, np.float64)
    D = A.shape[0] - 1
    C = np.float64(C)
    with np.errstate(all="ignore"):
        idx = np.arange(D)
        A[idx, idx] = A[idx, idx] + np.float64(1.0) / C
        rhs = np.array(g, np.float64)
        rhs[:D] = rhs[:D] + np.asarray(trial, np.float64)[:D] / C
        y, bad = host_cholesky_solve(A[None], rhs[None])
        dec = serial_sum(rhs * y[0])
    return y[0], dec, bad


def host_update(loss_blocks, delta, dec, C: float, threshold: float, max_iter: int, beta, trial, step, fstate, state):
    """One round of mmg_prop_update for one lab, in place on beta, trial, step (fp64 [M]), fstate (fp64 [4]) and state
    (int32 [8])."""
    if state[ACTIVE] == 0:
        return
    D = beta.size - 1
    with np.errstate(all="ignore"):
        F = np.float64(serial_sum(loss_blocks)) + np.float64(serial_sum(trial[:D] * trial[:D])) / (np.float64(2.0) * np.float64(C))
        started = state[STARTED] != 0
        if started:
            state[N_ITER] += 1
        fstate[3] = F
        if not started or dec <= threshold or F <= fstate[0]:
            fstate[0], fstate[1], fstate[2] = F, 1.0, dec
            state[STARTED] = 1
            if dec <= threshold:
                beta[:] = trial - delta
                state[CONVERGED], state[ACTIVE] = 1, 0
                return
            beta[:] = trial
            if state[N_ITER] >= max_iter:
                state[ACTIVE] = 0
            else:
                step[:] = delta
                trial[:] = beta - step
        else:
            state[HALVINGS] += 1
            fstate[1] = fstate[1] * 0.5
            if state[N_ITER] >= max_iter:
                state[ACTIVE] = 0
            else:
                trial[:] = beta - fstate[1] * step


def start_point(count, n: int, D: int):
    """-> (trial fp64 [L, D + 1], state int32 [L, 8], degenerate bool [L]): w = 0, b = logit(mean y); a lab nobody or
    everybody has is not active and gets b = -inf / +inf."""
    count = np.asarray(count, np.int64)
    L = count.size
    trial = np.zeros((L, D + 1))
    state = np.zeros((L, N_STATE), np.int32)
    degenerate = (count == 0) | (count == n)
    m = count.astype(np.float64) / np.float64(n)
    with np.errstate(all="ignore"):
        trial[:, D] = np.where(count == 0, -np.inf, np.where(count == n, np.inf, np.log(m / (1.0 - m))))
    state[:, ACTIVE] = ~degenerate
    return trial, state, degenerate


def host_fit(X, Y, mean, C: float, max_iter: int, tol: float):
    """The whole fit on the host -> (beta [L, M], fstate [L, 4], state [L, 8], degenerate [L])."""
    X = np.asarray(X, np.float32)
    Y = np.asarray(Y)
    n, D = X.shape
    L = Y.shape[1]
    trial, state, degenerate = start_point(Y.astype(bool).sum(0), n, D)
    beta, step, fstate = trial.copy(), np.zeros_like(trial), np.zeros((L, N_FSTATE))
    threshold = float(tol) * float(n)
    for j in range(L):
        for _ in range(max_iter + 1):
            if state[j, ACTIVE] == 0:
                break
            z, p, q, s, r, t = host_link(X, mean, Y[:, j], trial[j])
            H, g = host_moments(X, mean, s, r)
            delta, dec, bad = host_solve(H, g, trial[j], C)
            state[j, BAD] += bad
            host_update(host_loss_blocks(t), delta, dec, C, threshold, max_iter, beta[j], trial[j], step[j], fstate[j], state[j])
    return beta, fstate, state, degenerate


def host_predict(X, mean, coef) -> np.ndarray:
    """-> fp32 [n, L]: p of host_link for every lab, rounded once."""
    X = np.asarray(X, np.float32)
    out = np.empty((X.shape[0], coef.shape[0]), np.float32)
    for j in range(coef.shape[0]):
        out[:, j] = host_link(X, mean, np.zeros(X.shape[0], np.uint8), coef[j])[1].astype(np.float32)
    return out


PAIR_CHUNK = 256                      # MMG_PR_PAIR_CHUNK
PAIR_FIELDS = ("sum_w", "sum_w2", "sum_w_abs", "sum_w_sq", "sum_abs", "sum_sq")


def host_pair_terms(pred, target, p, cov_j, clip: float, stabilized: bool) -> np.ndarray:
    """The six terms of mmg_prop_pair_sums for pairs of one lab, operation by operation -> fp64 [6, m]."""
    with np.errstate(all="ignore"):
        e = np.asarray(pred, np.float32).astype(np.float64) - np.asarray(target, np.float32).astype(np.float64)
        ae, e2 = np.abs(e), e * e
        pc = np.maximum(np.asarray(p, np.float32).astype(np.float64), np.float64(clip))
        w = (np.float64(cov_j) / pc) if stabilized else (np.float64(1.0) / pc)
        return np.stack([w, w * w, w * ae, w * e2, ae, e2])


def host_chunk_sum(t) -> float:
    """One lab's terms in pair order: chunks of 256 (zeros behind the last pair), each by the tree v_l += v_{l+o},
    o = 128 .. 1, the chunk sums added from 0 in ascending order."""
    t = np.asarray(t, np.float64)
    chunks = (t.size + PAIR_CHUNK - 1) // PAIR_CHUNK
    if chunks == 0:
        return 0.0
    v = np.zeros(chunks * PAIR_CHUNK)
    v[:t.size] = t
    v = v.reshape(chunks, PAIR_CHUNK)
    o = PAIR_CHUNK // 2
    while o:
        v = v[:, :o] + v[:, o:2 * o]
        o //= 2
    return serial_sum(v[:, 0])


def host_pair_sums(pred, target, patient, lab, P, cov, clip: float, stabilized: bool):
    """-> (count int64 [L + 1], sums fp64 [L + 1, 6]): the arithmetic and the order of mmg_prop_pair_sums."""
    P = np.asarray(P, np.float32)
    n, L = P.shape
    patient, lab = np.asarray(patient, np.int64), np.asarray(lab, np.int64)
    ok = (lab >= 0) & (lab < L) & (patient >= 0) & (patient < n)
    count, sums = np.zeros(L + 1, np.int64), np.zeros((L + 1, len(PAIR_FIELDS)))
    for j in range(L):
        idx = np.flatnonzero(ok & (lab == j))                            # a stable sort by lab keeps the given order
        count[j] = idx.size
        if idx.size:
            terms = host_pair_terms(np.asarray(pred)[idx], np.asarray(target)[idx], P[patient[idx], j],
                                    cov[j] if stabilized else 1.0, clip, stabilized)
            sums[j] = [host_chunk_sum(t) for t in terms]
    count[L] = count[:L].sum()
    sums[L] = [serial_sum(sums[:L, f]) for f in range(len(PAIR_FIELDS))]
    return count, sums


def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


# ============================================================================ the device fit
class _DeviceFit:
    """The device tensors of one fit and ``round()``: link, moments, solve, update per batch of labs; nothing read back,
    capturable."""

    def __init__(self, X, mean, Y, trial, state, C, threshold, max_iter):
        from . import prop_ops
        self.ops = o = prop_ops
        dev = X.device
        n, D = (int(v) for v in X.shape)
        L = int(Y.shape[1])
        self.X, self.mean, self.Y, self.n, self.D, self.L = X, mean, Y, n, D, L
        self.C, self.threshold, self.max_iter = float(C), float(threshold), int(max_iter)
        batch = o.prop_batch(n, D)
        self.batches = [(j0, min(batch, L - j0)) for j0 in range(0, L, batch)]
        nb = self.batches[0][1]
        f64 = dict(dtype=torch.float64, device=dev)
        self.trial = torch.from_numpy(trial).to(dev)
        self.beta = self.trial.clone()
        self.step = torch.zeros(L, D + 1, **f64)
        self.fstate = torch.zeros(L, o.PR_FSTATE, **f64)
        self.state = torch.from_numpy(state).to(dev)
        self._sr = torch.empty(2 * nb * n, **f64)
        self._lossp = torch.empty(nb * o.link_blocks(n), **f64)
        self._H = torch.empty(nb * (D + 1) * (D + 1), **f64)
        self._g, self._delta, self._dec = (torch.empty(nb * (D + 1), **f64), torch.empty(nb * (D + 1), **f64),
                                           torch.empty(nb, **f64))

    def views(self, nb: int):
        n, M = self.n, self.D + 1
        blocks = self.ops.link_blocks(n)
        return (self._sr[:2 * nb * n].view(2, nb, n), self._lossp[:nb * blocks].view(nb, blocks),
                self._H[:nb * M * M].view(nb, M, M), self._g[:nb * M].view(nb, M), self._delta[:nb * M].view(nb, M),
                self._dec[:nb])

    def round(self):
        o = self.ops
        for j0, nb in self.batches:
            sr, lossp, H, g, delta, dec = self.views(nb)
            o.prop_link(self.X, self.mean, self.Y, j0, nb, self.trial, self.state, sr, lossp)
            o.prop_moments(self.X, self.mean, sr, self.L, j0, nb, self.state, H, g)
            o.prop_solve(H, g, self.trial, j0, self.C, self.state, delta, dec)
            o.prop_update(lossp, self.n, j0, delta, dec, self.C, self.threshold, self.max_iter, self.beta, self.trial,
                          self.step, self.fstate, self.state)

    def loss_and_brier(self, coef):
        """-> (sum of the loss terms, sum of r^2) per lab at ``coef``, fp64 [L] on the host: the figures of the report,
        not part of the fit."""
        o = self.ops
        loss, brier = [], []
        for j0, nb in self.batches:
            sr, lossp = self.views(nb)[:2]
            o.prop_link(self.X, self.mean, self.Y, j0, nb, coef, None, sr, lossp)
            loss.append(lossp.sum(1))
            brier.append((sr[1] * sr[1]).sum(1))
        return torch.cat(loss).cpu().numpy(), torch.cat(brier).cpu().numpy()


class LabPropensity:
    """``fit(features, observed)``, then ``predict_proba(features)`` -> fp32 [rows, labs].  ``observed`` is a bool / uint8
    [n, L] mask or an fp32 lab matrix whose NaN means "not measured" (``association.lab_matrix``).  After the fit:
    ``coef_`` [L, D], ``intercept_`` [L] (for the uncentred features), ``n_iter_``, ``converged_``, ``degenerate_``,
    ``halvings_``, ``decrement_``, and per lab ``deviance_`` (2 x the unpenalised loss), ``null_deviance_``, ``pseudo_r2_`` (McFadden;
    NaN for a degenerate lab) and ``brier_``."""

    def __init__(self, C: float = 1.0, max_iter: int = 25, tol: float = 1e-8):
        self.C, self.max_iter, self.tol = C, max_iter, tol
        self._st = None               # host: mean [D], beta [L, M] (centred), the per-lab figures
        self._dev = {}

    def _check_params(self):
        if not (isinstance(self.C, (int, float)) and np.isfinite(self.C) and self.C > 0):
            raise ValueError(f"C must be a positive finite number, got {self.C!r}")
        if not (isinstance(self.max_iter, int) and self.max_iter >= 1):
            raise ValueError(f"max_iter must be an int >= 1, got {self.max_iter!r}")
        if not (isinstance(self.tol, (int, float)) and np.isfinite(self.tol) and self.tol >= 0):
            raise ValueError(f"tol must be a finite number >= 0, got {self.tol!r}")

    @staticmethod
    def _check_shape(n: int, D: int, L: int, rows: int):
        if not 1 <= D <= MAX_FEATURES:
            raise ValueError(f"the features have {D} columns, outside [1, {MAX_FEATURES}]")
        if not 1 <= L <= MAX_LABS:
            raise ValueError(f"observed has {L} labs, outside [1, {MAX_LABS}]")
        if not 1 <= n < 2 ** 31:
            raise ValueError(f"the features have {n} rows, outside [1, 2^31)")
        if rows != n:
            raise ValueError(f"{n} rows of features but {rows} rows of observed")

    # ------------------------------------------------------------------ fit
    def fit(self, features, observed) -> "LabPropensity":
        self._check_params()
        self._dev = {}
        if _is_dev(features) != _is_dev(observed):
            raise ValueError("features and observed must both be HIP tensors or both be host arrays")
        for t, name in ((features, "features"), (observed, "observed")):
            if len(getattr(t, "shape", ())) != 2:
                raise ValueError(f"{name} must be a 2-D matrix")
        return self._fit_device(features, observed) if _is_dev(features) else self._fit_host(features, observed)

    def _fit_host(self, features, observed):
        from .association import _host_matrix, host_colstats
        X = _host_matrix(features)
        Y = _np(observed)
        Y = np.isfinite(Y) if Y.dtype.kind == "f" else Y != 0
        n, D = X.shape
        self._check_shape(n, D, Y.shape[1], Y.shape[0])
        if not np.isfinite(X).all():
            raise ValueError("features hold NaN or infinite cells: a propensity feature is dense and finite")
        mean = host_colstats(X)[1]
        beta, fstate, state, degenerate = host_fit(X, Y, mean, self.C, self.max_iter, self.tol)
        loss = np.zeros(Y.shape[1])
        brier = np.zeros(Y.shape[1])
        for j in np.flatnonzero(~degenerate):
            r, t = host_link(X, mean, Y[:, j], beta[j])[4:6]
            loss[j], brier[j] = serial_sum(host_loss_blocks(t)), float((r * r).sum())
        return self._finish(mean, beta, state, fstate, degenerate, Y.sum(0), n, loss, brier)

    def _fit_device(self, features, observed):
        from . import assoc_ops, prop_ops
        from .association import _dev_matrix
        X = _dev_matrix(features)
        n, D = (int(v) for v in X.shape)
        self._check_shape(n, D, int(observed.shape[1]), int(observed.shape[0]))
        if observed.dtype.is_floating_point:
            Y = prop_ops.prop_indicator(_dev_matrix(observed))
        else:
            Y = (observed != 0).view(torch.uint8) if observed.dtype != torch.uint8 else observed.clamp(max=1)
        L = int(Y.shape[1])
        fcount, mean, n_inf = assoc_ops.assoc_colstats(X)
        count = prop_ops.prop_count(Y)
        head = torch.cat([n_inf, fcount.min().reshape(1), count]).cpu().numpy()                 # the one read before the rounds
        if int(head[0]) or int(head[1]) < n:
            raise ValueError("features hold NaN or infinite cells: a propensity feature is dense and finite")
        count_h = head[2:].astype(np.int64)
        trial, state, degenerate = start_point(count_h, n, D)
        fit = _DeviceFit(X, mean, Y, trial, state, self.C, float(self.tol) * float(n), self.max_iter)
        for _ in range(self.max_iter + 1):
            fit.round()
        loss, brier = fit.loss_and_brier(fit.beta)
        self._dev[X.device] = dict(mean=mean, beta=fit.beta)
        return self._finish(mean.cpu().numpy(), fit.beta.cpu().numpy(), fit.state.cpu().numpy(), fit.fstate.cpu().numpy(),
                            degenerate, count_h, n,
                            np.where(degenerate, 0.0, loss), np.where(degenerate, 0.0, brier))

    def _finish(self, mean, beta, state, fstate, degenerate, count, n, loss, brier):
        bad = int(state[:, BAD].sum())
        if bad:
            raise FloatingPointError(f"{bad} pivots of the Newton systems were not positive")
        m = np.asarray(count, np.float64) / float(n)
        with np.errstate(all="ignore"):
            null = np.where(degenerate, 0.0, -2.0 * n * (m * np.log(m) + (1.0 - m) * np.log1p(-m)))
            dev = 2.0 * np.asarray(loss, np.float64)
            r2 = np.where(degenerate, np.nan, 1.0 - dev / null)
        self._st = dict(mean=np.asarray(mean, np.float64), beta=np.asarray(beta, np.float64),
                        n_iter=state[:, N_ITER].astype(np.int64), converged=state[:, CONVERGED] != 0,
                        halvings=state[:, HALVINGS].astype(np.int64), decrement=np.asarray(fstate[:, 2], np.float64),
                        degenerate=np.asarray(degenerate, bool),
                        deviance=dev, null_deviance=null, pseudo_r2=r2, brier=np.asarray(brier, np.float64) / float(n),
                        coverage=m)
        return self

    # ------------------------------------------------------------------ reading the fit
    def _fitted(self):
        if self._st is None:
            raise RuntimeError("LabPropensity: call fit() first")
        return self._st

    coef_ = property(lambda self: self._fitted()["beta"][:, :-1].copy())
    n_iter_ = property(lambda self: self._fitted()["n_iter"])
    converged_ = property(lambda self: self._fitted()["converged"])
    halvings_ = property(lambda self: self._fitted()["halvings"])
    decrement_ = property(lambda self: self._fitted()["decrement"])       # at the last accepted trial point
    degenerate_ = property(lambda self: self._fitted()["degenerate"])
    deviance_ = property(lambda self: self._fitted()["deviance"])
    null_deviance_ = property(lambda self: self._fitted()["null_deviance"])
    pseudo_r2_ = property(lambda self: self._fitted()["pseudo_r2"])
    brier_ = property(lambda self: self._fitted()["brier"])
    coverage_ = property(lambda self: self._fitted()["coverage"])

    @property
    def intercept_(self) -> np.ndarray:
        st = self._fitted()
        return st["beta"][:, -1] - st["beta"][:, :-1] @ st["mean"]

    def predict_proba(self, features):
        """-> fp32 [rows, L]: the propensity of every lab for every row (new patients included).  A HIP tensor runs the
        kernel."""
        st = self._fitted()
        D = st["mean"].size
        if len(getattr(features, "shape", ())) != 2 or features.shape[1] != D:
            raise ValueError(f"features must be [rows, {D}]")
        if _is_dev(features):
            from . import prop_ops
            from .association import _dev_matrix
            X = _dev_matrix(features)
            if not bool(torch.isfinite(X).all()):
                raise ValueError("features hold NaN or infinite cells: a propensity feature is dense and finite")
            if X.device not in self._dev:
                self._dev[X.device] = dict(mean=torch.from_numpy(st["mean"]).to(X.device),
                                           beta=torch.from_numpy(st["beta"]).to(X.device))
            d = self._dev[X.device]
            return prop_ops.prop_predict(X, d["mean"], d["beta"])
        from .association import _host_matrix
        X = _host_matrix(features)
        if not np.isfinite(X).all():
            raise ValueError("features hold NaN or infinite cells: a propensity feature is dense and finite")
        out = host_predict(X, st["mean"], st["beta"])
        return torch.from_numpy(out) if torch.is_tensor(features) else out

    # ------------------------------------------------------------------ state
    _KEYS = ("mean", "beta", "n_iter", "converged", "halvings", "decrement", "degenerate", "deviance", "null_deviance", "pseudo_r2",
             "brier", "coverage")

    def state_dict(self) -> dict:
        st = self._fitted()
        out = {k: torch.from_numpy(np.array(st[k])) for k in self._KEYS}
        out.update(C=float(self.C), max_iter=int(self.max_iter), tol=float(self.tol))
        return out

    def load_state_dict(self, state: dict) -> "LabPropensity":
        missing = [k for k in self._KEYS + ("C", "max_iter", "tol") if k not in state]
        if missing:
            raise KeyError(f"LabPropensity.load_state_dict: missing {missing}")
        st = {k: _np(state[k]).copy() for k in self._KEYS}
        L, M = st["beta"].shape if st["beta"].ndim == 2 else (0, 0)
        if st["mean"].shape != (M - 1,) or not 1 <= M - 1 <= MAX_FEATURES or not 1 <= L <= MAX_LABS \
                or any(st[k].shape != (L,) for k in self._KEYS[2:]):
            raise ValueError("LabPropensity.load_state_dict: inconsistent shapes")
        self.C, self.max_iter, self.tol = float(state["C"]), int(state["max_iter"]), float(state["tol"])
        self._st, self._dev = st, {}
        return self


# ============================================================================ features and the report
CODE_RELATIONS = (("diagnosis", ("patient", "has_diagnosis", "diagnosis")),
                  ("medication", ("patient", "has_medication", "medication")))


def _code_name(graph, node: str, idx: int) -> str:
    meta = graph[node].metadata if "metadata" in graph[node] else None
    label = meta[idx]["label"] if meta and idx in meta and "label" in meta[idx] else idx
    return f"{node}:{label}"


def measurement_features(graph, kind: str = "codes", max_features: int = MAX_FEATURES, model=None):
    """What is known about a patient besides the labs -> (features fp32 [patients, D], names).

    ``kind="codes"``: the patient x code 0 / 1 matrix of the ``max_features`` diagnoses and medications that the most
    patients have (ties go to the diagnosis, then to the smaller index), through ``association.lab_matrix`` over
    (patient, code, 1) and the indicator kernel.  Runs where the graph lives.

    ``kind="embedding"``: the patient rows of ``model.encode_nodes(graph)`` (at most 128 wide).  An embedding trained on
    has_lab edges HAS SEEN which labs exist for a patient: a propensity fitted on it is the propensity GIVEN THE MODEL,
    useful for weighting that model's errors, and not a test of missing-at-random."""
    if kind == "embedding":
        if model is None:
            raise ValueError('kind="embedding" needs the model')
        if getattr(model, "_comm", None) is not None:
            raise NotImplementedError("measurement_features on a patient-sharded model (dist.shard_model) is not supported")
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                x = model.encode_nodes(graph.to(next(model.parameters()).device))["patient"].float().contiguous()
        finally:
            model.train(was_training)
        if x.shape[1] > MAX_FEATURES:
            raise ValueError(f"the embedding is {x.shape[1]} wide, more than {MAX_FEATURES}")
        return x, [f"embedding:{a}" for a in range(x.shape[1])]
    if kind != "codes":
        raise ValueError(f'kind must be "codes" or "embedding", got {kind!r}')
    if not 1 <= int(max_features) <= MAX_FEATURES:
        raise ValueError(f"max_features must be in [1, {MAX_FEATURES}], got {max_features}")
    from .association import lab_matrix
    P = int(graph["patient"].num_nodes)
    counts, owner = [], []
    for node, rel in CODE_RELATIONS:
        if rel in graph.edge_types:
            V = int(graph[node].num_nodes)
            counts.append(torch.bincount(graph[rel].edge_index[1].cpu(), minlength=V)[:V])
            owner += [(node, rel, i) for i in range(V)]
    if not counts:
        raise ValueError("the graph has neither has_diagnosis nor has_medication edges")
    counts = torch.cat(counts).numpy()
    order = np.argsort(-counts, kind="mergesort")[:int(max_features)]
    order = order[counts[order] > 0]
    if order.size == 0:
        raise ValueError("no diagnosis or medication has a patient")
    pi, ci = [], []
    for node, rel in CODE_RELATIONS:
        if rel not in graph.edge_types:
            continue
        ei = graph[rel].edge_index
        column = torch.full((int(graph[node].num_nodes),), -1, dtype=torch.int64)
        for c, k in enumerate(order):
            if owner[k][0] == node:
                column[owner[k][2]] = c
        col = column.to(ei.device)[ei[1]]
        keep = col >= 0
        pi.append(ei[0][keep])
        ci.append(col[keep])
    pi, ci = torch.cat(pi), torch.cat(ci)
    ones = torch.ones(pi.numel(), dtype=torch.float32, device=pi.device)
    M = lab_matrix(pi, ci, ones, P, int(order.size))
    names = [_code_name(graph, owner[k][0], owner[k][2]) for k in order]
    if _is_dev(M):
        from . import prop_ops
        return prop_ops.prop_indicator(M, features=True)[1], names
    return np.isfinite(M).astype(np.float32), names


IPW_COLUMNS = ("lab", "n", "ess", "mae_ipw", "rmse_ipw", "mae", "rmse")


class IpwMetrics(NamedTuple):
    per_lab: pd.DataFrame             # lab, n, ess, mae_ipw, rmse_ipw, mae, rmse
    overall: dict                     # the same fields over all pairs
    count: np.ndarray                 # int64 [L + 1]
    sums: np.ndarray                  # fp64 [L + 1, 6]: PAIR_FIELDS


def ipw_metrics(predictions, targets, patient_indices, lab_indices, propensity, clip: float = 0.02,
                stabilized: bool = True, coverage=None, lab_names=None) -> IpwMetrics:
    """The error of ``predictions`` over the WHOLE patient x lab matrix, estimated from the measured pairs by weighting
    each with the inverse of its propensity: ``w = 1 / max(p, clip)``, or ``coverage_j / max(p, clip)`` when
    ``stabilized``.  ``propensity`` is fp32 [patients, labs] (``LabPropensity.predict_proba``); ``coverage`` (per lab,
    the share of patients that have it) defaults to the column means of ``propensity``, which a logistic fit with a free
    intercept makes equal to that share on its training rows.  Per lab and overall: ``n``, the effective sample size
    ``(sum w)^2 / sum w^2``, ``mae_ipw = sum w |e| / sum w``, ``rmse_ipw = sqrt(sum w e^2 / sum w)`` and the unweighted
    ``mae``, ``rmse``.  HIP tensors run ``mmg_prop_pair_sums``; numpy arrays the restatement."""
    if not (isinstance(clip, (int, float)) and 0.0 < clip <= 1.0):
        raise ValueError(f"clip must be in (0, 1], got {clip!r}")
    if len(getattr(propensity, "shape", ())) != 2:
        raise ValueError("propensity must be a [patients, labs] matrix")
    n, L = (int(v) for v in propensity.shape)
    if not 1 <= L <= MAX_LABS or not 1 <= n < 2 ** 31:
        raise ValueError(f"propensity is [{n}, {L}]: at most {MAX_LABS} labs and 2^31 - 1 patients")
    dev = _is_dev(propensity)
    given = (predictions, targets, patient_indices, lab_indices)
    if any(_is_dev(t) != dev for t in given):
        raise ValueError("predictions, targets, indices and propensity must all be HIP tensors or all be host arrays")
    if dev:
        from . import assoc_ops, prop_ops
        from .association import _dev_matrix
        pred, y = (t.detach().reshape(-1).float().contiguous() for t in (predictions, targets))
        pi, li = (t.reshape(-1).to(torch.int64).contiguous() for t in (patient_indices, lab_indices))
        m = pred.numel()
        if not (y.numel() == pi.numel() == li.numel() == m):
            raise ValueError("predictions, targets, patient_indices and lab_indices must have one entry per pair")
        if m and (int(pi.min()) < 0 or int(pi.max()) >= n or int(li.min()) < 0 or int(li.max()) >= L):
            raise ValueError(f"a patient index outside [0, {n}) or a lab index outside [0, {L})")
        P = _dev_matrix(propensity)
        if not bool(torch.isfinite(pred).all() & torch.isfinite(y).all()) or not bool(((P >= 0) & (P <= 1)).all()):
            raise ValueError("predictions and targets must be finite and every propensity in [0, 1]")
        if coverage is None:
            cov = assoc_ops.assoc_colstats(P)[1]
        else:
            cov = torch.as_tensor(_np(coverage), dtype=torch.float64).reshape(-1).to(P.device).contiguous()
        if cov.numel() != L:
            raise ValueError(f"coverage must hold {L} values")
        count, sums = prop_ops.prop_pair_sums(pred, y, pi, li, P, cov, float(clip), bool(stabilized))
        count, sums = count.cpu().numpy(), sums.cpu().numpy()
    else:
        from .association import host_colstats
        pred, y = (_np(t).reshape(-1).astype(np.float32) for t in (predictions, targets))
        pi, li = (_np(t).reshape(-1) for t in (patient_indices, lab_indices))
        m = pred.size
        if not (y.size == pi.size == li.size == m):
            raise ValueError("predictions, targets, patient_indices and lab_indices must have one entry per pair")
        if pi.dtype.kind not in "iu" or li.dtype.kind not in "iu":
            raise ValueError("patient_indices and lab_indices must hold integers")
        if m and (int(pi.min()) < 0 or int(pi.max()) >= n or int(li.min()) < 0 or int(li.max()) >= L):
            raise ValueError(f"a patient index outside [0, {n}) or a lab index outside [0, {L})")
        P = np.ascontiguousarray(_np(propensity), np.float32)
        if not (np.isfinite(pred).all() and np.isfinite(y).all()) or not ((P >= 0) & (P <= 1)).all():
            raise ValueError("predictions and targets must be finite and every propensity in [0, 1]")
        cov = host_colstats(P)[1] if coverage is None else np.asarray(_np(coverage), np.float64).reshape(-1)
        if cov.size != L:
            raise ValueError(f"coverage must hold {L} values")
        count, sums = host_pair_sums(pred, y, pi, li, P, cov, float(clip), bool(stabilized))
    with np.errstate(all="ignore"):
        cnt = count.astype(np.float64)
        table = dict(n=count, ess=sums[:, 0] * sums[:, 0] / sums[:, 1], mae_ipw=sums[:, 2] / sums[:, 0],
                     rmse_ipw=np.sqrt(sums[:, 3] / sums[:, 0]), mae=sums[:, 4] / cnt, rmse=np.sqrt(sums[:, 5] / cnt))
    from .analysis import _lab_name
    frame = pd.DataFrame({"lab": [_lab_name(lab_names, j) for j in range(L)], **{k: v[:L] for k, v in table.items()}})
    overall = {k: (int(v[L]) if k == "n" else float(v[L])) for k, v in table.items()}
    overall.update(clip=float(clip), stabilized=bool(stabilized))
    return IpwMetrics(frame, overall, count, sums)


def missingness_report(graph, output_dir, model=None, masker=None, split: str = "test", kind: str = "codes",
                       max_features: int = MAX_FEATURES, lab_names=None, clip: float = 0.02, stabilized: bool = True, **kw):
    """Fit a ``LabPropensity(**kw)`` of the graph's has_lab edges on ``measurement_features(graph, kind)`` and write

    * ``lab_propensity.csv``: per lab ``lab, coverage, pseudo_r2, brier, n_iter, converged, degenerate`` and the five
      largest |coefficients| with their feature names (``top1_feature, top1_coef, ..``);
    * ``lab_propensity_coefficients.csv``: ``lab, intercept`` and one column per feature.

    * with a ``model`` and its ``masker``, ``ipw_metrics.csv``: ``lab, n, ess, mae_ipw, rmse_ipw, mae, rmse`` of the model's
      predictions on the ``split`` pairs, per lab and in a last row "overall": the error estimate for the whole matrix
      (``ipw_metrics`` with ``clip``, ``stabilized``) beside the usual one for the measured cells.

    Runs where the graph lives, or with a model on the model's device.  -> (LabPropensity, {"propensity", "coefficients"
    and, with a model, "ipw": frames}).  A patient-sharded model is refused."""
    from .association import LAB_EDGE, _graph_names, _lab_name, lab_matrix
    if model is not None and getattr(model, "_comm", None) is not None:
        raise NotImplementedError("missingness_report on a patient-sharded model (dist.shard_model) is not supported: the "
                                  "forward's collectives need every rank; report with an unsharded model")
    if (model is None) != (masker is None):
        raise ValueError("ipw_metrics.csv needs both the model and the masker; the two propensity tables need neither")
    if model is not None:
        graph = graph.to(next(model.parameters()).device)
    feats, names = measurement_features(graph, kind, max_features, model=model)
    ei = graph[LAB_EDGE].edge_index
    if _is_dev(feats) and not ei.is_cuda:
        ei = ei.to(feats.device)
    X = lab_matrix(ei[0], ei[1], torch.ones(ei.shape[1], dtype=torch.float32, device=ei.device),
                   int(graph["patient"].num_nodes), int(graph["lab"].num_nodes))
    prop = LabPropensity(**kw).fit(feats, X)
    lab_names = lab_names if lab_names is not None else _graph_names(graph)
    L = prop.coef_.shape[0]
    labs = [_lab_name(lab_names, j) for j in range(L)]
    coef = prop.coef_
    rows = []
    for j in range(L):
        row = dict(lab=labs[j], coverage=prop.coverage_[j], pseudo_r2=prop.pseudo_r2_[j], brier=prop.brier_[j],
                   n_iter=int(prop.n_iter_[j]), converged=bool(prop.converged_[j]), degenerate=bool(prop.degenerate_[j]))
        top = np.argsort(-np.abs(coef[j]), kind="mergesort")[:5]
        for k in range(5):
            row[f"top{k + 1}_feature"] = names[top[k]] if k < top.size else ""
            row[f"top{k + 1}_coef"] = coef[j, top[k]] if k < top.size else np.nan
        rows.append(row)
    frames = {"propensity": pd.DataFrame(rows),
              "coefficients": pd.concat([pd.DataFrame({"lab": labs, "intercept": prop.intercept_}),
                                         pd.DataFrame(coef, columns=names)], axis=1)}
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    frames["propensity"].to_csv(out / "lab_propensity.csv", index=False)
    frames["coefficients"].to_csv(out / "lab_propensity_coefficients.csv", index=False)
    if model is not None:
        from .conformal import _predict_split
        _, pred, y, pi, li = _predict_split(model, graph, masker, split)
        ipw = ipw_metrics(pred, y, pi, li, prop.predict_proba(feats), clip=clip, stabilized=stabilized,
                          coverage=prop.coverage_, lab_names=lab_names)
        frames["ipw"] = pd.concat([ipw.per_lab, pd.DataFrame([dict(lab="overall", **{k: ipw.overall[k] for k in
                                                                                    IPW_COLUMNS[1:]})])], ignore_index=True)
        frames["ipw"].to_csv(out / "ipw_metrics.csv", index=False)
    logging.info(f"  Saved lab propensity tables to {out}")
    return prop, frames
