"""Lab imputation by low-rank matrix completion: every patient ``i`` gets a vector ``u_i`` and every lab ``l`` a vector
``v_l`` (``rank`` values each), the value of lab ``l`` for patient ``i`` is ``center_l + u_i . v_l``, and the factors
minimise ``F = sum (y - u.v)^2 + reg (|U|^2 + |V|^2)`` over the observed cells by alternating least squares.  It is the
model under test -- learnable node embeddings, message passing, a pair head -- with the message passing taken out, and
the comparator every EHR imputation benchmark reports beside the mean, nearest-neighbour and chained-equations ones.
It works on the observed (patient, lab, value) triples alone: O(pairs . rank^2) a round, up to 2048 labs.

Definitions (this module's numpy functions are the definition; ``tests/mf_ref.py`` restates them in loops, math.fsum and
80-bit arithmetic):

* ``count`` and ``center`` are the observed count and the fp64 mean of the observed values of every lab;
  ``y = value - center_lab``.  A lab with ``count == 0`` is INACTIVE: its factor is zero, its column of
  ``impute_matrix`` and its ``predict`` are NaN (``KNNLabImputer``'s and ``ChainedLabImputer``'s behaviour).
* the pairs are held in two segment orderings (``host_index``): by patient, labs ascending, and by lab, patients
  ascending, each with row pointers.
* one half-sweep (``host_half_sweep``) solves for every segment ``s`` of one ordering, with ``F`` the factors of the
  other side, ``A_s = sum f f^T + reg I``, ``b_s = sum f y``, ``x_s = A_s^{-1} b_s`` (``host_normal``, ``host_solve``:
  the package's one Cholesky solve, ``cholesky.host_cholesky_solve``, operation by operation, no fused
  multiply-add).  An empty segment gets the zero vector; a pivot that is not ``> 0`` is counted.  The patient side and
  the lab side are the same computation.
* a round is the patient half-sweep, then the lab half-sweep, then the objective (``host_objective``: the squared
  residuals, ``|U|^2``, ``|V|^2``; ``F`` is recorded in ``history_``).  The fit stops after the round with ``F_prev - F <
  tol F_prev`` or after ``max_iter`` rounds; ``tol = 0`` never stops early.  One more patient half-sweep closes the
  fit, so that the stored ``U`` is the fold-in of the stored ``V`` -- what ``transform`` computes for new patients.
* the start is ``V0 = default_rng(seed).standard_normal((n_labs, rank)) * 0.1`` (or ``init``), inactive rows zeroed.
* a prediction is ``clip(center_l + sum_k u_ik v_lk, min_value, max_value)``, ``k`` ascending, no fused multiply-add,
  rounded once to fp32.

HIP tensors run the kernels of libmmgnn_mf.so (csrc/mf.hip), whose sums follow the fixed order of include/mmgnn_mf.h;
the host reads 24 bytes a round, or nothing until the end with ``tol = 0``.  numpy arrays (and CPU tensors) run the
float64 restatement of this module, which is the checker and never a silent substitute for the kernels.  Plain ALS
only: no weighted-lambda, no bias terms beyond the centre, no implicit feedback, no SGD, no nuclear-norm SoftImpute.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .analysis import _is_dev
from .cholesky import host_cholesky_solve

MAX_LABS = 2048                       # MMG_MF_MAX_LABS
MAX_RANK = 32                         # MMG_MF_MAX_RANK


# ============================================================================ the numpy restatement
def host_index(patient, lab, value, n_patients: int, n_labs: int, center=None) -> dict:
    """The triples -> both orderings (numpy's stable sorts), count, center and y; the arrays of mmg_mf_index."""
    p, lb = np.asarray(patient, np.int64), np.asarray(lab, np.int64)
    v = np.asarray(value, np.float32)
    op = np.lexsort((lb, p))
    ol = np.lexsort((p, lb))
    count = np.bincount(lb, minlength=n_labs).astype(np.int64)
    if center is None:
        tot = np.bincount(lb[ol], weights=v[ol].astype(np.float64), minlength=n_labs)
        center = np.divide(tot, count, out=np.zeros(n_labs), where=count > 0)
    center = np.ascontiguousarray(center, np.float64)
    y = v.astype(np.float64) - center[lb]
    ptr = lambda seg, n: np.concatenate([[0], np.cumsum(np.bincount(seg, minlength=n))]).astype(np.int64)    # noqa: E731
    return dict(p_ptr=ptr(p, n_patients), p_idx=lb[op].astype(np.int32), p_val=v[op], p_y=y[op],
                l_ptr=ptr(lb, n_labs), l_idx=p[ol].astype(np.int32), l_y=y[ol], count=count, center=center,
                n_patients=int(n_patients), n_labs=int(n_labs))


def _segment_ids(ptr) -> np.ndarray:
    ptr = np.asarray(ptr, np.int64)
    return np.repeat(np.arange(ptr.size - 1), np.diff(ptr))


def host_normal(ptr, idx, y, other, reg: float):
    """-> (A fp64 [segments, r, r], b fp64 [segments, r]): every segment's sum f f^T + reg I and sum f y, the pairs in
    stored order; A exactly symmetric."""
    other = np.asarray(other, np.float64)
    S, r = np.asarray(ptr).size - 1, other.shape[1]
    seg = _segment_ids(ptr)
    f = other[np.asarray(idx, np.int64)]
    y = np.asarray(y, np.float64)
    A, b = np.zeros((S, r, r)), np.zeros((S, r))
    for k in range(r):
        for l in range(k + 1):
            A[:, k, l] = A[:, l, k] = np.bincount(seg, weights=f[:, k] * f[:, l], minlength=S)
        A[:, k, k] = A[:, k, k] + np.float64(reg)
        b[:, k] = np.bincount(seg, weights=f[:, k] * y, minlength=S)
    return A, b


def host_solve(A, b):
    """x = A^{-1} b for every system of A [S, r, r], b [S, r]: the arithmetic of mmg_mf_half_sweep's solve, operation
    by operation (``host_cholesky_solve``) -> (x fp64 [S, r], pivots not > 0)."""
    return host_cholesky_solve(A, b)


def host_half_sweep(ptr, idx, y, other, reg: float):
    """-> (x fp64 [segments, r], pivots not > 0): the ridge solution of every segment against ``other``."""
    A, b = host_normal(ptr, idx, y, other, reg)
    x, bad = host_solve(A, b)
    x[np.diff(np.asarray(ptr, np.int64)) == 0] = 0.0
    return x, bad


def _dots(u_rows, v_rows) -> np.ndarray:
    t = np.zeros(np.broadcast_shapes(u_rows.shape[:-1], v_rows.shape[:-1]))
    for k in range(u_rows.shape[-1]):
        t = t + u_rows[..., k] * v_rows[..., k]
    return t


def host_objective(ix: dict, U, V):
    """-> (sum of the squared residuals over the pairs, |U|^2, |V|^2)."""
    pat = _segment_ids(ix["p_ptr"])
    d = ix["p_y"] - _dots(U[pat], V[ix["p_idx"].astype(np.int64)])
    return float((d * d).sum()), float((U * U).sum()), float((V * V).sum())


def host_predict(patient, lab, U, V, center, count, lo: float, hi: float) -> np.ndarray:
    """fp32 [n]: clip(center[lab] + U[patient] . V[lab], lo, hi); NaN for a lab nobody has."""
    patient, lab = np.asarray(patient, np.int64), np.asarray(lab, np.int64)
    v = np.minimum(np.maximum(center[lab] + _dots(U[patient], V[lab]), lo), hi).astype(np.float32)
    v[np.asarray(count)[lab] == 0] = np.float32(np.nan)
    return v


def host_impute(rows, U, V, center, count, lo: float, hi: float, ix: dict) -> np.ndarray:
    """fp32 [rows, n_labs]: every lab's prediction for the patients ``rows``, their own values passed through."""
    rows = np.arange(U.shape[0]) if rows is None else np.asarray(rows, np.int64)
    v = np.minimum(np.maximum(center[None, :] + _dots(U[rows][:, None, :], V[None, :, :]), lo), hi).astype(np.float32)
    v[:, np.asarray(count) == 0] = np.float32(np.nan)
    ptr = ix["p_ptr"]
    for j, i in enumerate(rows):
        q = slice(int(ptr[i]), int(ptr[i + 1]))
        v[j, ix["p_idx"][q]] = ix["p_val"][q]
    return v


def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _objective_value(parts, reg: float) -> float:
    return float(parts[0]) + float(reg) * (float(parts[1]) + float(parts[2]))


def _check_triples(patient_indices, lab_indices, values, n_patients: int, n_labs: int):
    """The checks of ``KNNLabImputer.fit``: ranges, NaN, duplicates, one device -> (patient int64, lab int64, value
    fp32) as tensors on the inputs' device."""
    if not 1 <= int(n_labs) <= MAX_LABS:
        raise ValueError(f"n_labs must be in [1, {MAX_LABS}], got {n_labs}")
    if not 1 <= int(n_patients) < 2 ** 31:
        raise ValueError(f"n_patients must be in [1, 2^31), got {n_patients}")
    if _is_dev(values):
        as_t = lambda x: x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))           # noqa: E731
    else:
        as_t = lambda x: torch.as_tensor(_np(x))                                                # noqa: E731
    p, lab, v = as_t(patient_indices), as_t(lab_indices), as_t(values).detach()
    for t, name in ((p, "patient_indices"), (lab, "lab_indices")):
        if t.dim() != 1:
            raise ValueError(f"{name} must be 1-D, got shape {list(t.shape)}")
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"{name} must hold integers, got {t.dtype}")
    if v.dim() == 2 and v.shape[1] == 1:
        v = v[:, 0]
    if not (p.numel() == lab.numel() == v.numel()) or v.dim() != 1:
        raise ValueError(f"patient_indices, lab_indices and values must have one entry per cell, got "
                         f"{p.numel()}, {lab.numel()} and shape {list(v.shape)}")
    if not (p.device == lab.device == v.device):
        raise ValueError(f"inputs on different devices: {p.device}, {lab.device}, {v.device}")
    if p.numel() >= 2 ** 31 - 1:
        raise ValueError(f"{p.numel()} pairs, outside [0, 2^31)")
    p, lab = p.to(torch.int64).contiguous(), lab.to(torch.int64).contiguous()
    if p.numel():
        if int(p.min()) < 0 or int(p.max()) >= int(n_patients):
            raise ValueError(f"patient index outside [0, {int(n_patients)})")
        if int(lab.min()) < 0 or int(lab.max()) >= int(n_labs):
            raise ValueError(f"lab index outside [0, {int(n_labs)})")
    if bool(torch.isnan(v).any()):
        raise ValueError("values hold NaN: NaN marks a missing cell and cannot be an observation")
    if bool(torch.isinf(v).any()):
        raise ValueError("values hold infinite cells: a lab value is finite")
    key = p * int(n_labs) + lab
    if torch.unique(key).numel() != key.numel():
        raise ValueError("duplicate (patient, lab) pairs")
    return p, lab, v.to(torch.float32).contiguous()


class _DeviceALS:
    """The device tensors of one fit and ``round(r)``: two half-sweeps and the objective, nothing read back, capturable."""

    def __init__(self, ix, V0: torch.Tensor, reg: float, max_iter: int):
        from . import mf_ops
        self.ops, self.ix, self.reg = mf_ops, ix, float(reg)
        dev, r = V0.device, V0.shape[1]
        self.V = V0
        self.U = torch.zeros(ix.n_patients, r, dtype=torch.float64, device=dev)
        self.obj = torch.zeros(max_iter, 3, dtype=torch.float64, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int64, device=dev)

    def patient_half(self):
        self.ops.mf_half_sweep(self.ix.p_ptr, self.ix.p_idx, self.ix.p_y, self.V, self.reg, self.U, self.bad)

    def lab_half(self):
        self.ops.mf_half_sweep(self.ix.l_ptr, self.ix.l_idx, self.ix.l_y, self.U, self.reg, self.V, self.bad)

    def round(self, r: int):
        self.patient_half()
        self.lab_half()
        self.ops.mf_objective(self.ix, self.U, self.V, self.obj[r])


class LowRankLabImputer:
    """``fit`` the (patient, lab, value) triples (or ``fit_matrix`` a dense matrix, NaN = missing), then
    ``impute_matrix`` / ``predict`` / ``transform``.  A lab nobody has stays NaN."""

    def __init__(self, rank: int = 8, reg: float = 1.0, max_iter: int = 20, tol: float = 1e-4, seed: int = 0, init=None,
                 min_value: float = -np.inf, max_value: float = np.inf):
        self.rank, self.reg, self.max_iter, self.tol, self.seed, self.init = rank, reg, max_iter, tol, seed, init
        self.min_value, self.max_value = min_value, max_value
        self.n_iter_: Optional[int] = None
        self.history_: list = []
        self._state = None            # host: V, center, count
        self._dev = {}                # device -> the same as device tensors
        self._fit = None              # the training side: the index and U (host dict / device objects); None when loaded
        self._tensor_out = False

    # ------------------------------------------------------------------ validation
    def _check_params(self):
        if not (isinstance(self.rank, (int, np.integer)) and 1 <= self.rank <= MAX_RANK):
            raise ValueError(f"rank must be an int in [1, {MAX_RANK}], got {self.rank!r}")
        if not (isinstance(self.reg, (int, float)) and np.isfinite(self.reg) and self.reg > 0):
            raise ValueError(f"reg must be a positive finite number, got {self.reg!r}")
        if not (isinstance(self.max_iter, (int, np.integer)) and self.max_iter >= 1):
            raise ValueError(f"max_iter must be an int >= 1, got {self.max_iter!r}")
        if not (isinstance(self.tol, (int, float)) and np.isfinite(self.tol) and self.tol >= 0):
            raise ValueError(f"tol must be a finite number >= 0, got {self.tol!r}")
        lo, hi = float(self.min_value), float(self.max_value)
        if np.isnan(lo) or np.isnan(hi) or not lo < hi:
            raise ValueError(f"min_value must be below max_value, got {self.min_value!r} and {self.max_value!r}")

    def _start(self, n_labs: int, count) -> np.ndarray:
        if self.init is None:
            V0 = np.random.default_rng(self.seed).standard_normal((n_labs, int(self.rank))) * 0.1
        else:
            V0 = np.array(_np(self.init), np.float64)
            if V0.shape != (n_labs, int(self.rank)):
                raise ValueError(f"init must have shape [{n_labs}, {self.rank}], got {list(V0.shape)}")
            if not np.isfinite(V0).all():
                raise ValueError("init holds values that are not finite")
        if count is not None:
            V0[np.asarray(count) == 0] = 0.0
        return np.ascontiguousarray(V0)

    # ------------------------------------------------------------------ fit
    def fit(self, patient_indices, lab_indices, values, n_patients: int, n_labs: int, center=None) -> "LowRankLabImputer":
        """The triples under the checks of ``KNNLabImputer.fit``.  HIP tensors run the kernels, anything else the numpy
        restatement.  center: fp64 [n_labs] to use instead of the lab means."""
        self._check_params()
        p, lab, v = _check_triples(patient_indices, lab_indices, values, n_patients, n_labs)
        n_patients, n_labs = int(n_patients), int(n_labs)
        if center is not None:
            center = np.ascontiguousarray(_np(center), np.float64)
            if center.shape != (n_labs,) or not np.isfinite(center).all():
                raise ValueError(f"center must hold {n_labs} finite values")
        self._dev, self.history_ = {}, []
        if v.is_cuda:
            self._tensor_out = True
            return self._fit_device(p, lab, v, n_patients, n_labs, center)
        self._tensor_out = torch.is_tensor(values)
        return self._fit_host(p.numpy(), lab.numpy(), v.numpy(), n_patients, n_labs, center)

    def fit_matrix(self, X, center=None) -> "LowRankLabImputer":
        """A dense [patients, labs] matrix, NaN = missing."""
        t = X.detach() if torch.is_tensor(X) else torch.as_tensor(np.asarray(X))
        if t.dim() != 2:
            raise ValueError(f"X must be a 2-D matrix [patients, labs], got shape {list(t.shape)}")
        cells = torch.nonzero(~torch.isnan(t))
        p, lab = cells[:, 0].contiguous(), cells[:, 1].contiguous()
        v = t[p, lab]
        if not torch.is_tensor(X):
            p, lab, v = p.numpy(), lab.numpy(), v.numpy()
        return self.fit(p, lab, v, int(t.shape[0]), int(t.shape[1]), center=center)

    def _stop(self, F_prev, F) -> bool:
        return self.tol > 0 and F_prev is not None and F_prev - F < float(self.tol) * F_prev

    def _fit_host(self, p, lab, v, n_patients, n_labs, center):
        ix = host_index(p, lab, v, n_patients, n_labs, center)
        V = self._start(n_labs, ix["count"])
        reg, bad, F_prev = float(self.reg), 0, None
        for _ in range(int(self.max_iter)):
            U, b1 = host_half_sweep(ix["p_ptr"], ix["p_idx"], ix["p_y"], V, reg)
            V, b2 = host_half_sweep(ix["l_ptr"], ix["l_idx"], ix["l_y"], U, reg)
            bad += b1 + b2
            F = _objective_value(host_objective(ix, U, V), reg)
            self.history_.append(F)
            if self._stop(F_prev, F):
                break
            F_prev = F
        U, b1 = host_half_sweep(ix["p_ptr"], ix["p_idx"], ix["p_y"], V, reg)
        self._refuse_pivots(bad + b1)
        self.n_iter_ = len(self.history_)
        self._state = dict(V=V, center=ix["center"], count=ix["count"])
        self._fit = dict(ix=ix, U=U)
        return self

    def _fit_device(self, p, lab, v, n_patients, n_labs, center):
        from . import mf_ops
        dev = v.device
        c = None if center is None else torch.from_numpy(center).to(dev)
        ix = mf_ops.mf_index(p, lab, v, n_patients, n_labs, center=c)
        V0 = torch.from_numpy(self._start(n_labs, None)).to(dev)
        V0 = torch.where(ix.count[:, None] > 0, V0, torch.zeros_like(V0)).contiguous()      # nothing is read back
        als = _DeviceALS(ix, V0, self.reg, int(self.max_iter))
        F_prev = None
        for r in range(int(self.max_iter)):
            als.round(r)
            if self.tol > 0:
                F = _objective_value(als.obj[r].cpu().numpy(), self.reg)        # the round's one read: 24 bytes
                self.history_.append(F)
                if self._stop(F_prev, F):
                    break
                F_prev = F
        als.patient_half()
        if not self.tol > 0:
            self.history_ = [_objective_value(o, self.reg) for o in als.obj.cpu().numpy()]
        self._refuse_pivots(int(als.bad.item()))
        self.n_iter_ = len(self.history_)
        self._state = dict(V=als.V.cpu().numpy(), center=ix.center.cpu().numpy(), count=ix.count.cpu().numpy())
        self._dev[dev] = dict(V=als.V, center=ix.center, count=ix.count)
        self._fit = dict(ix=ix, U=als.U)
        return self

    @staticmethod
    def _refuse_pivots(bad: int):
        if bad:
            raise FloatingPointError(f"{bad} pivots of the ridge systems were not positive")

    # ------------------------------------------------------------------ reading the fit
    def _check_fitted(self):
        if self._state is None:
            raise RuntimeError("LowRankLabImputer: call fit() first")

    def _check_trained(self):
        self._check_fitted()
        if self._fit is None:
            raise RuntimeError("LowRankLabImputer: a loaded state has no training data; use transform()")

    def _on_device(self) -> bool:
        return self._fit is not None and torch.is_tensor(self._fit["U"])

    def _out(self, a):
        return torch.from_numpy(a) if self._tensor_out and not torch.is_tensor(a) else a

    @property
    def patient_factors_(self):
        self._check_trained()
        return self._out(self._fit["U"])

    @property
    def lab_factors_(self):
        self._check_fitted()
        return self._dev[self._fit["U"].device]["V"] if self._on_device() else self._out(self._state["V"])

    def _index(self, t, what: str, hi: int):
        name = f"{what}_indices"
        if self._on_device():
            t = torch.as_tensor(t)
            if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f"{name} must be a 1-D integer tensor")
            t = t.to(self._fit["U"].device).to(torch.int64).contiguous()
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= hi):
                raise ValueError(f"{what} index outside [0, {hi})")
            return t
        t = _np(t)
        if t.ndim != 1 or t.dtype.kind not in "iu":
            raise ValueError(f"{name} must be a 1-D integer array")
        if t.size and (int(t.min()) < 0 or int(t.max()) >= hi):
            raise ValueError(f"{what} index outside [0, {hi})")
        return t.astype(np.int64)

    def _clip(self):
        return float(self.min_value), float(self.max_value)

    def impute_matrix(self, patient_indices=None):
        """-> fp32 [rows, n_labs]: every lab of every requested training patient (default: all, in order)."""
        self._check_trained()
        ix, U = self._fit["ix"], self._fit["U"]
        rows = None if patient_indices is None else self._index(patient_indices, "patient", int(U.shape[0]))
        lo, hi = self._clip()
        if self._on_device():
            d = self._dev[U.device]
            return self._fit_ops().mf_impute_matrix(rows, U, d["V"], d["center"], d["count"], lo, hi, ix.p_ptr, ix.p_idx,
                                                    ix.p_val)
        st = self._state
        return self._out(host_impute(rows, U, st["V"], st["center"], st["count"], lo, hi, ix))

    @staticmethod
    def _fit_ops():
        from . import mf_ops
        return mf_ops

    def predict(self, patient_indices, lab_indices):
        """-> fp32 [n]: the reconstruction at each (patient, lab) cell of the training patients."""
        self._check_trained()
        U = self._fit["U"]
        p = self._index(patient_indices, "patient", int(U.shape[0]))
        lab = self._index(lab_indices, "lab", int(self._state["count"].size))
        if len(p) != len(lab):
            raise ValueError(f"{len(p)} patients but {len(lab)} labs")
        lo, hi = self._clip()
        if self._on_device():
            d = self._dev[U.device]
            return self._fit_ops().mf_predict_pairs(p, lab, U, d["V"], d["center"], d["count"], lo, hi)
        st = self._state
        return self._out(host_predict(p, lab, U, st["V"], st["center"], st["count"], lo, hi))

    def transform(self, patient_indices, lab_indices, values, n_new: int):
        """Fold ``n_new`` new patients in against the stored lab factors (one patient half-sweep over their triples) ->
        their imputed matrix fp32 [n_new, n_labs].  HIP tensors run the kernels."""
        self._check_fitted()
        st = self._state
        L = int(st["count"].size)
        p, lab, v = _check_triples(patient_indices, lab_indices, values, n_new, L)
        lo, hi = self._clip()
        if v.is_cuda:
            ops = self._fit_ops()
            d = self._device_state(v.device)
            ix = ops.mf_index(p, lab, v, int(n_new), L, center=d["center"])
            U = torch.zeros(int(n_new), d["V"].shape[1], dtype=torch.float64, device=v.device)
            bad = torch.zeros(1, dtype=torch.int64, device=v.device)
            ops.mf_half_sweep(ix.p_ptr, ix.p_idx, ix.p_y, d["V"], float(self.reg), U, bad)
            self._refuse_pivots(int(bad.item()))
            return ops.mf_impute_matrix(None, U, d["V"], d["center"], d["count"], lo, hi, ix.p_ptr, ix.p_idx, ix.p_val)
        ix = host_index(p.numpy(), lab.numpy(), v.numpy(), int(n_new), L, center=st["center"])
        U, bad = host_half_sweep(ix["p_ptr"], ix["p_idx"], ix["p_y"], st["V"], float(self.reg))
        self._refuse_pivots(bad)
        out = host_impute(None, U, st["V"], st["center"], st["count"], lo, hi, ix)
        return torch.from_numpy(out) if torch.is_tensor(values) else out

    def _device_state(self, device):
        if device not in self._dev:
            st = self._state
            self._dev[device] = {k: torch.from_numpy(np.ascontiguousarray(st[k])).to(device) for k in ("V", "center", "count")}
        return self._dev[device]

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        """Everything ``transform`` needs, as CPU tensors and plain values: no training data."""
        self._check_fitted()
        st = self._state
        out = {k: torch.from_numpy(np.array(st[k])) for k in ("V", "center", "count")}
        out.update(rank=int(self.rank), reg=float(self.reg), max_iter=int(self.max_iter), tol=float(self.tol),
                   seed=int(self.seed), min_value=float(self.min_value), max_value=float(self.max_value),
                   n_iter=int(self.n_iter_), history=list(self.history_))
        return out

    def load_state_dict(self, state: dict) -> "LowRankLabImputer":
        need = ("V", "center", "count", "rank", "reg", "max_iter", "tol", "seed", "min_value", "max_value", "n_iter",
                "history")
        missing = [k for k in need if k not in state]
        if missing:
            raise KeyError(f"LowRankLabImputer.load_state_dict: missing {missing}")
        st = dict(V=np.ascontiguousarray(_np(state["V"]), np.float64), center=_np(state["center"]).astype(np.float64),
                  count=_np(state["count"]).astype(np.int64))
        L, r = st["count"].size, int(state["rank"])
        if st["V"].shape != (L, r) or st["center"].shape != (L,) or not 1 <= L <= MAX_LABS or not 1 <= r <= MAX_RANK:
            raise ValueError("LowRankLabImputer.load_state_dict: inconsistent shapes")
        self.rank, self.reg, self.max_iter, self.tol = r, float(state["reg"]), int(state["max_iter"]), float(state["tol"])
        self.seed, self.init = int(state["seed"]), None
        self.min_value, self.max_value = float(state["min_value"]), float(state["max_value"])
        self.n_iter_, self.history_ = int(state["n_iter"]), list(state["history"])
        self._state, self._dev, self._fit = st, {}, None
        return self
