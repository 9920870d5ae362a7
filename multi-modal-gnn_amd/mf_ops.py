"""ctypes binding and typed entry points of libmmgnn_mf.so (C ABI: include/mmgnn_mf.h; csrc/mf.hip): the index of the
(patient, lab, value) triples, the half-sweep, the objective and the predictions of lab imputation by low-rank matrix
completion, a library of its own beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the header, and
every call goes through ``ops._call``.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback behind these
calls (the numpy restatement of mmgnn/lowrank.py serves numpy inputs and checks the kernels; it is never a silent
substitute for them).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import ops

BINDING = ops.satellite("mf", globals())    # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

MF_MAX_LABS = DEFINES["MMG_MF_MAX_LABS"]
MF_MAX_RANK = DEFINES["MMG_MF_MAX_RANK"]
MF_CHUNK = DEFINES["MMG_MF_CHUNK"]
MF_SPLIT = DEFINES["MMG_MF_SPLIT"]


def mf_plan(length: int):
    """How a segment of ``length`` pairs is summed (mmg_mf_plan, a host function) -> (path, chunks)."""
    path, chunks = C.c_int(0), C.c_int64(0)
    ops.check(load().mmg_mf_plan(int(length), C.byref(path), C.byref(chunks)), "mmg_mf_plan")
    return int(path.value), int(chunks.value)


@dataclass
class MFIndex:
    """Both orderings of the pairs (mmg_mf_index), on one device."""
    p_ptr: torch.Tensor               # int64 [n_patients + 1]
    p_idx: torch.Tensor               # int32 [nnz]: the lab of every pair, by patient
    p_val: torch.Tensor               # fp32 [nnz]: the values, by patient
    p_y: torch.Tensor                 # fp64 [nnz]: value - center
    l_ptr: torch.Tensor               # int64 [n_labs + 1]
    l_idx: torch.Tensor               # int32 [nnz]: the patient of every pair, by lab
    l_y: torch.Tensor
    count: torch.Tensor               # int64 [n_labs]
    center: torch.Tensor              # fp64 [n_labs]
    n_patients: int = 0
    n_labs: int = 0

    @property
    def nnz(self) -> int:
        return int(self.p_idx.numel())


def _bytes(nbytes: int) -> int:
    """A workspace size for ``_call`` (which takes the shared workspace of the tensors' device, after it has refused a
    tensor that is not on one): never under 256 bytes."""
    return max(int(nbytes), 256)


def _vec(t: torch.Tensor, n: int, name: str, what: str):
    if not torch.is_tensor(t) or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous vector of {n} values")


def _factors(F: torch.Tensor, rows: int, name: str, what: str) -> int:
    if not torch.is_tensor(F) or F.dim() != 2 or F.shape[0] != rows or not F.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous [{rows}, rank] tensor")
    return int(F.shape[1])


def mf_index(patient: torch.Tensor, lab: torch.Tensor, value: torch.Tensor, n_patients: int, n_labs: int,
             center=None) -> MFIndex:
    """The triples (int64, int64, fp32; the caller has checked them) -> both orderings, count, center and y.
    center: fp64 [n_labs] to use instead of the lab means."""
    nnz, dev = int(value.numel()), value.device
    _vec(patient, nnz, "patient", "mf_index")
    _vec(lab, nnz, "lab", "mf_index")
    _vec(value, nnz, "value", "mf_index")
    if center is not None:
        _vec(center, int(n_labs), "center", "mf_index")
    e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)              # noqa: E731
    ix = MFIndex(e(n_patients + 1, torch.int64), e(nnz, torch.int32), e(nnz, torch.float32), e(nnz, torch.float64),
                 e(n_labs + 1, torch.int64), e(nnz, torch.int32), e(nnz, torch.float64), e(n_labs, torch.int64),
                 e(n_labs, torch.float64), int(n_patients), int(n_labs))
    _call("mmg_mf_index", patient, lab, value, nnz, int(n_patients), int(n_labs), center, ix.p_ptr, ix.p_idx, ix.p_val,
          ix.p_y, ix.l_ptr, ix.l_idx, ix.l_y, ix.count, ix.center,
          ws=_bytes(load().mmg_mf_index_ws_bytes(nnz, int(n_patients), int(n_labs))))
    return ix


def mf_half_sweep(ptr: torch.Tensor, idx: torch.Tensor, y: torch.Tensor, other: torch.Tensor, reg: float,
                  out: torch.Tensor, bad: torch.Tensor, normal_out=None):
    """out [segments, r] = every segment's ridge solution against the factors ``other`` [m, r]; bad (int64 [1]) += the
    pivots that were not positive; normal_out (fp64 [segments, r * r + r], tests only): every A | b
    (mmg_mf_half_sweep)."""
    segments, nnz = int(ptr.numel()) - 1, int(idx.numel())
    r = _factors(other, int(other.shape[0]), "other", "mf_half_sweep")
    _vec(y, nnz, "y", "mf_half_sweep")
    if _factors(out, segments, "out", "mf_half_sweep") != r:
        raise ValueError(f"mf_half_sweep: out has rank {out.shape[1]}, other {r}")
    if normal_out is not None and (tuple(normal_out.shape) != (segments, r * r + r) or not normal_out.is_contiguous()):
        raise ValueError(f"mf_half_sweep: normal_out must be a contiguous [{segments}, {r * r + r}] tensor")
    _call("mmg_mf_half_sweep", ptr, idx, y, segments, nnz, other, int(other.shape[0]), r, float(reg), out, bad, normal_out,
          ws=_bytes(load().mmg_mf_half_sweep_ws_bytes(segments, nnz, r)))


def mf_objective(ix: MFIndex, U: torch.Tensor, V: torch.Tensor, out: torch.Tensor):
    """out (fp64 [3]) = the squared residuals over the pairs, |U|^2, |V|^2 (mmg_mf_objective)."""
    r = _factors(U, ix.n_patients, "U", "mf_objective")
    if _factors(V, ix.n_labs, "V", "mf_objective") != r:
        raise ValueError(f"mf_objective: U has rank {r}, V {V.shape[1]}")
    _vec(out, 3, "out", "mf_objective")
    _call("mmg_mf_objective", ix.p_ptr, ix.p_idx, ix.p_y, ix.nnz, ix.n_patients, ix.n_labs, U, V, r, out,
          ws=_bytes(load().mmg_mf_objective_ws_bytes(ix.nnz, ix.n_patients, ix.n_labs, r)))


def mf_predict_pairs(patient: torch.Tensor, lab: torch.Tensor, U: torch.Tensor, V: torch.Tensor, center: torch.Tensor,
                     count: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """fp32 [n]: clip(center[lab] + U[patient] . V[lab]), NaN for a lab nobody has (mmg_mf_predict_pairs)."""
    n = int(patient.numel())
    _vec(patient, n, "patient", "mf_predict_pairs")
    _vec(lab, n, "lab", "mf_predict_pairs")
    r = _factors(U, int(U.shape[0]), "U", "mf_predict_pairs")
    L = int(V.shape[0])
    if _factors(V, L, "V", "mf_predict_pairs") != r:
        raise ValueError(f"mf_predict_pairs: U has rank {r}, V {V.shape[1]}")
    _vec(center, L, "center", "mf_predict_pairs")
    _vec(count, L, "count", "mf_predict_pairs")
    out = torch.empty(n, dtype=torch.float32, device=U.device)
    _call("mmg_mf_predict_pairs", patient, lab, n, U, int(U.shape[0]), V, L, r, center, count, float(lo), float(hi), out)
    return out


def mf_impute_matrix(rows, U: torch.Tensor, V: torch.Tensor, center: torch.Tensor, count: torch.Tensor, lo: float,
                     hi: float, p_ptr: torch.Tensor, p_idx: torch.Tensor, p_val: torch.Tensor) -> torch.Tensor:
    """fp32 [rows, n_labs]: every lab's prediction for the patients ``rows`` (int64; None: all of U's), their own values
    passed through (mmg_mf_impute_matrix)."""
    P = int(U.shape[0])
    r = _factors(U, P, "U", "mf_impute_matrix")
    L = int(V.shape[0])
    if _factors(V, L, "V", "mf_impute_matrix") != r:
        raise ValueError(f"mf_impute_matrix: U has rank {r}, V {V.shape[1]}")
    _vec(center, L, "center", "mf_impute_matrix")
    _vec(count, L, "count", "mf_impute_matrix")
    _vec(p_ptr, P + 1, "p_ptr", "mf_impute_matrix")
    nnz = int(p_idx.numel())
    _vec(p_val, nnz, "p_val", "mf_impute_matrix")
    n_rows = P if rows is None else int(rows.numel())
    if rows is not None:
        _vec(rows, n_rows, "rows", "mf_impute_matrix")
    out = torch.empty(n_rows, L, dtype=torch.float32, device=U.device)
    _call("mmg_mf_impute_matrix", rows, n_rows, U, P, V, L, r, center, count, float(lo), float(hi), p_ptr, p_idx, p_val,
          nnz, out, L)
    return out
