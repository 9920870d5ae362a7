"""Typed Python entry points over the C ABI (include/mmgnn.h): one function per exported op.

PyTorch is plumbing here -- it owns device memory and the stream; every computation below is a
hand-written HIP kernel in libmmgnn.so.  All tensors must live on a HIP device, be contiguous and
fp32 (indices int32 unless stated); violations raise instead of silently copying.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import (BnFinT, FwdEpiT, HeadGradT, HeadT, NextBnT, PairSavedT, PrologueT, RelT, SmallBnBwdT, SmallBnT, SmallFwdT, SmallWgradT, SumJobT, WgradReduceT, BnBwdT, BnBwdWgradT,
                   check)

BN_MOMENTUM = 0.1
BN_EPS = 1e-5
L2_EPS = 1e-12


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor], dtype=torch.float32, name="tensor", contiguous=True):
    """Device pointer of a tensor for a descriptor field, or for an argument whose dtype or layout the prototype cannot
    give (None: NULL).  dtype: one, or a tuple of accepted ones.  contiguous=False: the tensor may be a strided view (the
    caller passes its strides on)."""
    if t is None:
        return None
    where = f"{name}: " if name else ""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not t.is_cuda:
        raise _lib.MmgError(f"{where}expected a HIP device tensor, got {t.device} (no CPU fallback)")
    if t.dtype not in dtypes:
        raise TypeError(f"{where}expected {dtypes[0]}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return C.c_void_p(t.data_ptr())


def _plan(params):
    """What becomes of each parameter of a prototype: "stream", "ws" or "ws_bytes" (filled by _call), (header's name,
    accepted torch dtypes) for a pointer to a scalar the dtype table knows, None for the rest (passed as given)
    -> (plan, number of arguments the caller gives)."""
    has_ws = any(p[0] == "ws" for p in params)
    plan = []
    for pname, base, depth in params:
        if pname == "stream" or (has_ws and pname in ("ws", "ws_bytes")):
            plan.append(pname)
        elif depth == 1 and base in _lib.TORCH_DTYPES:
            plan.append((pname, tuple(getattr(torch, d) for d in _lib.TORCH_DTYPES[base])))
        else:
            plan.append(None)
    return plan, sum(1 for how in plan if not isinstance(how, str))


_BOUND = {}     # binding -> {symbol: _plan of its prototype}


def _plans(binding):
    """The plans of a binding's prototypes: decided once, from its header alone."""
    if binding not in _BOUND:
        _BOUND[binding] = {sym: _plan(params) for sym, params in binding.params.items()}
    return _BOUND[binding]


_PLANS = _plans(_lib.MAIN)


def _call(name, *args, ws=None, names=None, binding=None):
    """The one path into every library: `args` are the parameters of the prototype of `name` (in the header of `binding`;
    None: libmmgnn.so's, include/mmgnn.h) without stream, ws and ws_bytes.  A torch.Tensor handed to a scalar pointer
    parameter is converted under the header's dtype and parameter name (names: {header's name: the name a refusal uses
    instead}); tensors on different devices are refused; everything else -- None, numbers, ctypes values, a pointer made by
    _p -- passes through.  ws: a byte count (the shared workspace() on the device of the first tensor argument) or the
    call's own uint8 tensor.  The stream is the current one; the return code goes through check()."""
    plan, n_given = (_PLANS if binding is None else _plans(binding))[name]
    if len(args) != n_given:
        raise TypeError(f"{name}: takes {n_given} arguments besides ws and stream, got {len(args)}")
    if ws is not None and "ws" not in plan:
        raise TypeError(f"{name}: takes no workspace")
    out, dev, given = [], None, iter(args)
    for how in plan:
        a = (0 if how == "ws_bytes" else None) if isinstance(how, str) else next(given)       # ws=None: NULL, 0
        if how is not None and isinstance(a, torch.Tensor):
            t, a = a, _p(a, how[1], names.get(how[0], how[0]) if names else how[0])
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise ValueError(f"{name}: {how[0]} is on {t.device}, the tensors before it on {dev}")
        out.append(a)
    for i, how in enumerate(plan):              # after the conversions: a refused tensor costs no workspace
        if how == "stream":
            out[i] = _stream()
        elif how == "ws" and ws is not None:
            if not isinstance(ws, torch.Tensor):
                if dev is None:
                    raise _lib.MmgError(f"{name}: no tensor argument names the device of the workspace")
                ws = workspace(ws, dev)
            out[i], out[i + 1] = _p(ws, torch.uint8, "ws"), ws.numel()
    check(getattr(binding.load() if binding else _lib.load(), name)(*out), name)


def satellite(stem, namespace):
    """The binding of libmmgnn_<stem>.so, made by the one line of its <stem>_ops.py that hands in its globals(): they
    get LIB_PATH, HEADER_PATH, DEFINES, STRUCTS, SIGNATURES, PARAMS, every MMG_* define, load (the library, once, after
    libmmgnn.so) and _call (the _call above into this library).  The header is parsed here; no library is loaded."""
    b = _lib.Binding(stem)
    namespace.update(b.defines, LIB_PATH=b.lib_path, HEADER_PATH=b.header_path, DEFINES=b.defines, STRUCTS=b.structs,
                     SIGNATURES=b.signatures, PARAMS=b.params, load=b.load,
                     _call=lambda name, *args, **kw: _call(name, *args, binding=b, **kw))
    return b


# ------------------------------------------------------------------------------------------
# optional per-op timing (bench.py): HIP events recorded on the stream the kernels are launched on
class OpProfiler:
    """Collects (op, ms, algorithmic bytes, flops) per call; `only` restricts it to some op names."""

    def __init__(self, only=None):
        self.only = set(only) if only else None
        self.rows = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, nbytes, flops in self.rows:
            d = out.setdefault(name, dict(calls=0, ms=0.0, bytes=0, flops=0, shapes={}))
            ms = e0.elapsed_time(e1)
            d["calls"] += 1
            d["ms"] += ms
            d["bytes"] += nbytes
            d["flops"] += flops
            # launches of one op with the same algorithmic size are one kernel shape
            sh = d["shapes"].setdefault((nbytes, flops), dict(calls=0, ms=0.0, bytes=nbytes, flops=flops))
            sh["calls"] += 1
            sh["ms"] += ms
        return out


_PROF: Optional[OpProfiler] = None


def set_profiler(p: Optional[OpProfiler]):
    global _PROF
    _PROF = p


def _pb(name):
    if _PROF is None or (_PROF.only is not None and name not in _PROF.only):
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _pe(tok, name, nbytes=0, flops=0):
    if tok is None:
        return
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    _PROF.rows.append((name, tok, e, int(nbytes), int(flops)))


PROBE_TAGS = {_lib.MMG_PROBE_LINEAR_FWD: "linear_fwd", _lib.MMG_PROBE_LINEAR_WGRAD: "linear_wgrad",
              _lib.MMG_PROBE_LINEAR_WGRAD_REDUCE: "linear_wgrad_reduce", _lib.MMG_PROBE_GATHER: "gather_rows",
              _lib.MMG_PROBE_SCATTER: "scatter_rows", _lib.MMG_PROBE_SCATTER_REDUCE: "scatter_reduce",
              _lib.MMG_PROBE_PAIR_FWD: "pair_head_fwd", _lib.MMG_PROBE_PAIR_BWD: "pair_head_bwd",
              _lib.MMG_PROBE_BN_BWD_STATS: "bn_bwd_stats", _lib.MMG_PROBE_BN_BWD_APPLY: "bn_bwd_apply",
              _lib.MMG_PROBE_ELEMENTWISE: "elementwise", _lib.MMG_PROBE_PAIR_DENSE_FWD: "pair_head_dense_fwd",
              _lib.MMG_PROBE_KNN_IMPUTE: "knn_impute"}


def probe_arm(n: int):
    """Measurement hook: the next n big-kernel launches (any host thread) carry their own HIP start / stop event pair."""
    _call("mmg_probe_arm", int(n))


PROBE_NAME_LEN = _lib.MMG_PROBE_NAME_LEN


def probe_read(cap: int = 1 << 16):
    """-> list of (ms, family name, M, N, K, flags, kernel symbol) of the probed launches (flags: 1 accumulate, 4 prologue, 8 rowscale, 16 BatchNorm backward staged in the GEMM, 32 L2-norm epilogue, 64 L2-norm backward staged, 128 two upstream gradients, 256 row-list upstream gradient, 2048 the dual linear forward: N = both outputs, 4096 the weight gradient rides along the data gradient: linear_dgrad_wgrad, 8192 the masked dx store, 16384 the dual backward: linear_bnbwd_dual, 32768 a compact second problem rides in the launch: linear_l2norm_fwd_rider / linear_l2bwd with a rider)."""
    import numpy as np
    ms = np.zeros(cap, np.float32); tag = np.zeros(cap, np.int32); M = np.zeros(cap, np.int64)
    N = np.zeros(cap, np.int32); K = np.zeros(cap, np.int32); fl = np.zeros(cap, np.int32)
    names = np.zeros(cap * PROBE_NAME_LEN, np.uint8)
    n = _lib.load().mmg_probe_read(ms.ctypes.data, tag.ctypes.data, M.ctypes.data, N.ctypes.data, K.ctypes.data,
                                   fl.ctypes.data, names.ctypes.data, cap)
    nm = names.reshape(cap, PROBE_NAME_LEN)
    return [(float(ms[i]), PROBE_TAGS.get(int(tag[i]), str(int(tag[i]))), int(M[i]), int(N[i]), int(K[i]), int(fl[i]),
             bytes(nm[i]).split(b"\0", 1)[0].decode("ascii", "replace")) for i in range(n)]


def probe_grids(cap: int = 1 << 16):
    """-> list of ((gridDim.x, y, z), blockDim.x) of the launches the LAST probe_read returned, in its order: the grid of a
    persistent kernel tells how many tiles each of its workgroups walked."""
    import numpy as np
    grid = np.zeros((cap, 3), np.uint32); block = np.zeros(cap, np.uint32)
    n = _lib.load().mmg_probe_grids(grid.ctypes.data, block.ctypes.data, cap)
    return [((int(grid[i, 0]), int(grid[i, 1]), int(grid[i, 2])), int(block[i])) for i in range(n)]


_WS = {}              # key -> [buffer, handed out during a stream capture?]
_WS_RETIRED = []      # outgrown workspaces a captured hipGraph may hold the address of: never handed back


def workspace(nbytes: int, device) -> torch.Tensor:
    """Growable scratch per (device, host thread, stream).  Reuse is stream-ordered: an op runs on the current stream,
    and neither two host threads nor two streams (the model overlaps its vocab-side work on a side stream) share a
    buffer.  Growth is geometric (at least twice the old size: a sweep over growing shapes retires O(log n) buffers), and
    an outgrown buffer is only kept alive if it was ever handed out DURING a stream capture -- a graph recorded then replays
    kernels that write to it; one that no capture has seen goes back to the allocator."""
    import threading
    d = torch.device(device)
    key = (d.index if d.index is not None else torch.cuda.current_device(), threading.get_ident(),
           torch.cuda.current_stream().cuda_stream)
    ent = _WS.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if ent is None or ent[0].numel() < nbytes:
        old = 0
        if ent is not None:
            old = ent[0].numel()
            if ent[1]:
                # a step captured earlier on this stream replays kernels that write to the old buffer: if it went back to
                # the allocator, the next tensor placed there (an index list, say) would be scribbled over by the replay
                _WS_RETIRED.append(ent[0])
        ent = [torch.empty(max(int(nbytes), 2 * old, 1 << 20), dtype=torch.uint8, device=device), False]
        _WS[key] = ent
    if capturing:
        ent[1] = True
    return ent[0]


def _ws(nbytes: int, device):
    """The workspace() of a satellite library's call: never under 256 bytes."""
    return workspace(max(int(nbytes), 256), device)


def _edges(bin_edges):
    """Degree-bin edges -> (host array of doubles, number of bins)."""
    e = [float(x) for x in bin_edges]
    return (C.c_double * len(e))(*e), len(e) - 1


def _index_pair(patient: torch.Tensor, lab: torch.Tensor, n: int, what: str):
    """The two index tensors of the pairs as untyped pointers + their width; int64 or int32, both the same."""
    if patient.dtype != lab.dtype or patient.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"{what}: patient and lab indices must both be int64 or both int32, got {patient.dtype} / {lab.dtype}")
    if patient.numel() != n or lab.numel() != n:
        raise ValueError(f"{what}: {patient.numel()} patient and {lab.numel()} lab indices for {n} pairs")
    return _p(patient, patient.dtype, "patient"), _p(lab, lab.dtype, "lab"), patient.element_size()


@dataclass
class Pro:
    """Prologue dropout(act(x*scale+shift)) applied on load (mmg_prologue_t).  relu: False / True, or an MMG_ACT_* code
    (MMG_ACT_LEAKY_RELU, MMG_ACT_ELU: the materialising and backward kernels only)."""
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    relu: int = 0
    p: float = 0.0
    seed: int = 0
    site: int = 0
    row_offset: int = 0
    seed_dev: Optional[torch.Tensor] = None     # int64 [1] on the device: overrides `seed` at run time (hipGraph replays)

    def c(self):
        return PrologueT(_p(self.scale, name="pro.scale"), _p(self.shift, name="pro.shift"), int(self.relu),
                         float(self.p), int(self.seed) & 0xFFFFFFFFFFFFFFFF, int(self.site), int(self.row_offset),
                         _p(self.seed_dev, torch.int64, "pro.seed_dev"))


def _pro(pro: Optional[Pro]):
    return C.byref(pro.c()) if pro is not None else None


# ------------------------------------------------------------------------------------------ CSR
def csr_build(edge_index: torch.Tensor, n_rows: int, sort_row: int):
    """-> (rowptr int32 [n_rows+1], col int32 [E], perm int32 [E]); see mmg_csr_build."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2,E], got {tuple(edge_index.shape)}")
    E = int(edge_index.shape[1])
    dev = edge_index.device
    rowptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    col = torch.empty(E, dtype=torch.int32, device=dev)
    perm = torch.empty(E, dtype=torch.int32, device=dev)
    _call("mmg_csr_build", edge_index, E, n_rows, sort_row, rowptr, col, perm,
          ws=_lib.load().mmg_csr_build_ws_bytes(E, n_rows))
    return rowptr, col, perm


def row_degree(rowptr: torch.Tensor):
    n = rowptr.numel() - 1
    deg = torch.empty(n, dtype=torch.int32, device=rowptr.device)
    inv = torch.empty(n, dtype=torch.float32, device=rowptr.device)
    _call("mmg_row_degree", rowptr, n, deg, inv)
    return deg, inv


def col_degree(col: torch.Tensor, n_cols: int):
    cnt = torch.empty(n_cols, dtype=torch.int32, device=col.device)
    inv = torch.empty(n_cols, dtype=torch.float32, device=col.device)
    _call("mmg_col_degree", col, col.numel(), n_cols, cnt, inv)
    return cnt, inv


# ------------------------------------------------------------------------------------- aggregates
@dataclass
class Rel:
    rowptr: torch.Tensor
    col: torch.Tensor
    n_cols: int
    rowscale: Optional[torch.Tensor] = None
    colscale: Optional[torch.Tensor] = None
    table: Optional[torch.Tensor] = None
    out: Optional[torch.Tensor] = None
    simple: bool = False          # no duplicate (row, col) pair (MMG_REL_SIMPLE)
    mask_t: Optional[torch.Tensor] = None     # bit planes of the adjacency (rel_mask_build), simple relations only
    mask_r: Optional[torch.Tensor] = None     # the same, row-major (gather side)


def _agg_bytes(rels, n_rows, D, accumulate):
    """Algorithmic (compulsory) bytes of one fused aggregate launch: every index once, every distinct
    feature row once (the patient tensor is counted ONCE for the fused relations)."""
    b = 4 * D * n_rows * (2 if accumulate else 1)
    for r in rels:
        b += 4 * r.col.numel() + 4 * (n_rows + 1) + 4 * D * r.n_cols
        if r.rowscale is not None:
            b += 4 * n_rows
        if r.colscale is not None:
            b += 4 * r.n_cols
    return b


def _rels(rels: Sequence[Rel], D: int, need_table=False, need_out=False):
    if not 1 <= len(rels) <= _lib.MMG_MAX_REL:
        raise ValueError(f"1..{_lib.MMG_MAX_REL} relations per launch")
    arr = (RelT * len(rels))()
    for i, r in enumerate(rels):
        if need_table and (r.table is None or tuple(r.table.shape) != (r.n_cols, D)):
            raise ValueError(f"relation {i}: table must be [{r.n_cols},{D}]")
        if need_out and (r.out is None or tuple(r.out.shape) != (r.n_cols, D)):
            raise ValueError(f"relation {i}: out must be [{r.n_cols},{D}]")
        arr[i] = RelT(_p(r.rowptr, torch.int32), _p(r.col, torch.int32), _p(r.rowscale), _p(r.colscale),
                      _p(r.table), _p(r.out), r.n_cols, _lib.MMG_REL_SIMPLE if r.simple else 0,
                      _p(r.mask_t, torch.int64) if r.simple else None,
                      _p(r.mask_r, torch.int64) if r.simple else None)
    return arr


def rel_mask_build(rowptr: torch.Tensor, col: torch.Tensor, n_cols: int):
    """Bit planes of a SIMPLE CSR relation (mmg_rel_mask_build) -> (mask_t, mask_r), int64 storage each:
    mask_t [ceil(n_rows/64)][pad32(n_cols)][2] words (scatter side), mask_r [n_rows][2][pad32(n_cols)/16] uint16
    fields (gather side)."""
    lib = _lib.load()
    n_rows = rowptr.numel() - 1
    words = lib.mmg_rel_mask_words(n_rows, n_cols)
    mask_t = torch.empty(max(words, 1), dtype=torch.int64, device=rowptr.device)
    mask_r = torch.empty(max(words, 1), dtype=torch.int64, device=rowptr.device)
    _call("mmg_rel_mask_build", rowptr, col, n_rows, n_cols, mask_t,
          _p(mask_r, torch.int64, "mask_r"))          # uint16_t fields in int64 storage: no dtype to derive
    return mask_t, mask_r


def _bn_fin(count: int, N: int, device, bn):
    """bn = (gamma, beta, running_mean, running_var, n_updates) -> (mmg_bn_fin_t, the BNFold its launch fills)."""
    gamma, beta, rm, rv, n_updates = bn
    st = torch.empty(4, N, dtype=torch.float32, device=device)
    fin = BnFinT(int(count), _p(gamma), _p(beta), _p(rm), _p(rv), int(n_updates), BN_MOMENTUM, BN_EPS,
                 _p(st[0]), _p(st[1]), _p(st[2]), _p(st[3]))
    return fin, BNFold(st[0], st[1], st[2], st[3], int(count), True)


EPI_NONE, EPI_STATS, EPI_NEXT_BN, EPI_L2 = (_lib.MMG_EPI_NONE, _lib.MMG_EPI_STATS, _lib.MMG_EPI_NEXT_BN,
                                            _lib.MMG_EPI_L2)      # mmg_fwd_epi_t.mode


def _fwd_epi(what: str, M: int, N: int, device, with_stats=False, bn=None, next_bn: Optional["NextBN"] = None, l2=False):
    """The epilogue of one linear_fwd / gather_rows / linear_l2norm_fwd call (mmg_fwd_epi_t; it keeps what it points to
    alive) -> (descriptor or None, what the call returns after its output: (), (sums,), (sums, BNFold) or (rn,))."""
    if next_bn is not None:
        if bn is not None or with_stats:
            raise ValueError(f"{what}: next_bn excludes the forward statistics")
        nbt, sums = _next_bn(next_bn, M, N)
        e = FwdEpiT(EPI_NEXT_BN, next=C.pointer(nbt))
        e._keep = nbt
        return e, (sums,)
    if l2:
        rn = torch.empty(M, device=device)
        return FwdEpiT(EPI_L2, rnorm=_p(rn), eps=L2_EPS), (rn,)
    if bn is None and not with_stats:
        return None, ()
    sums = torch.empty(2, N, dtype=torch.float64, device=device)
    ws = workspace(_lib.load().mmg_epi_ws_bytes(M, N), device)
    fin, fold = _bn_fin(M, N, device, bn) if bn is not None else (None, None)
    e = FwdEpiT(EPI_STATS, col_sums=_p(sums, torch.float64), fin=C.pointer(fin) if fin is not None else None,
                ws=_p(ws, torch.uint8), ws_bytes=ws.numel())
    e._keep = (fin, ws)
    return e, (sums,) if fold is None else (sums, fold)


def gather_rows(rels: Sequence[Rel], n_rows: int, D: int, out: torch.Tensor, accumulate: bool, with_stats: bool = False,
                bn=None, next_bn: Optional["NextBN"] = None):
    """with_stats: also return fp64 [2,D] = (column sums, column sums of squares) of the final `out`.
    bn = (gamma, beta, running_mean, running_var, n_updates): also fold the training-mode BatchNorm of `out` in the launch
    that sums the statistics -> (out, sums, BNFold).
    next_bn: -> (out, the statistics of the BatchNorm backward that consumes out), see NextBN."""
    if tuple(out.shape) != (n_rows, D):
        raise ValueError("gather_rows: out shape")
    for r in rels:
        if r.rowptr.numel() != n_rows + 1:
            raise ValueError("gather_rows: rowptr length")
    arr = _rels(rels, D, need_table=True)
    _tok = _pb("gather_rows")
    epi, extra = _fwd_epi("gather_rows", n_rows, D, out.device, with_stats, bn, next_bn)
    _call("mmg_gather_rows", arr, len(rels), n_rows, D, out, int(accumulate), C.byref(epi) if epi is not None else None)
    _pe(_tok, "gather_rows", _agg_bytes(rels, n_rows, D, accumulate) + (4 * D * n_rows if next_bn is not None else 0), 0)
    return (out,) + extra if extra else out


def scatter_rows(rels: Sequence[Rel], n_rows: int, D: int, x: torch.Tensor):
    """Writes every rel.out ([n_cols, D])."""
    if tuple(x.shape) != (n_rows, D):
        raise ValueError("scatter_rows: x shape")
    for r in rels:
        if r.rowptr.numel() != n_rows + 1:
            raise ValueError("scatter_rows: rowptr length")
    arr = _rels(rels, D, need_out=True)
    nb = _lib.load().mmg_scatter_rows_ws_bytes(arr, len(rels), n_rows, D)
    _tok = _pb("scatter_rows")
    _call("mmg_scatter_rows", arr, len(rels), n_rows, D, x, ws=nb)
    _pe(_tok, "scatter_rows", _agg_bytes(rels, n_rows, D, False), 0)


# ------------------------------------------------------------------------------------------ dense
def linear_fwd(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None, pro: Optional[Pro] = None,
               out: Optional[torch.Tensor] = None, accumulate: bool = False, w_kn: bool = False,
               with_stats: bool = False, bn=None, next_bn: Optional["NextBN"] = None):
    """out[M,N] (+)= pro(x)[M,K] @ W[N,K]^T + bias;  w_kn: W is stored [K,N] (out = x @ W), read in place.
    next_bn: -> (out, the statistics of the BatchNorm backward that consumes out), see NextBN.
    with_stats: also return fp64 [2,N] = (column sums, column sums of squares) of out, from the GEMM epilogue.
    bn = (gamma, beta, running_mean, running_var, n_updates): also fold the training-mode BatchNorm of `out` in the launch
    that sums the statistics -> (out, sums, BNFold)."""
    return _linear_fwd(x, W, bias, pro, out, accumulate, w_kn, with_stats=with_stats, bn=bn, next_bn=next_bn)


def _lin_flags(accumulate, w_kn) -> int:
    return (_lib.MMG_LIN_ACCUMULATE if accumulate else 0) | (_lib.MMG_LIN_W_KN if w_kn else 0)


def _linear_fwd(x, W, bias, pro, out, accumulate, w_kn, **epi):
    """The one call behind linear_fwd and linear_l2norm_fwd (mmg_linear_fwd; epi: the options of _fwd_epi)."""
    M, K = x.shape
    N = W.shape[1] if w_kn else W.shape[0]
    if (W.shape[0] if w_kn else W.shape[1]) != K:
        raise ValueError(f"linear_fwd: W {tuple(W.shape)} vs x {tuple(x.shape)}")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (M, N):
        raise ValueError("linear_fwd: out shape")
    _tok = _pb("linear_fwd")
    desc, extra = _fwd_epi("linear_fwd", M, N, x.device, **epi)
    _call("mmg_linear_fwd", x, _pro(pro), W, bias, out, M, N, K, _lin_flags(accumulate, w_kn),
          C.byref(desc) if desc is not None else None, names={"X": "x", "Y": "out"})
    nbn = epi.get("next_bn") is not None          # + the next BatchNorm's y
    _pe(_tok, "linear_fwd", 4 * (M * K + N * K + M * N * (1 + int(accumulate) + int(nbn))), 2 * M * N * K)
    return (out,) + extra if extra else out


def linear_fwd_dual_supported(M: int, N: int, K: int) -> bool:
    return bool(_lib.load().mmg_linear_fwd_dual_supported(M, N, K))


def linear_fwd_dual(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], pro0: Pro, pro1: Pro, bn0=None, bn1=None):
    """The same layer under two dropout masks in one launch (mmg_linear_fwd_dual): pro0 and pro1 differ in their site
    alone.  -> ((out0, sums0[, BNFold0]), (out1, sums1[, BNFold1])): what linear_fwd(x, W, bias, pro=pro_c, with_stats=True
    / bn=bn_c) returns, pass 0's call before pass 1's, bit for bit.  bn0 / bn1 as linear_fwd's bn: both or neither."""
    M, K = x.shape
    N = W.shape[0]
    if W.shape[1] != K:
        raise ValueError(f"linear_fwd_dual: W {tuple(W.shape)} vs x {tuple(x.shape)}")
    if (bn0 is None) != (bn1 is None):
        raise ValueError("linear_fwd_dual: a BatchNorm fold for both passes or for neither")
    outs = [torch.empty(M, N, dtype=torch.float32, device=x.device) for _ in range(2)]
    nb = (_lib.load().mmg_epi_ws_bytes(M, N) + 255) // 256 * 256
    ws = workspace(2 * nb + 256, x.device)             # one half per pass: the two sets of partial rows live side by side
    descs, extras = [], []
    for c, bn in enumerate((bn0, bn1)):
        sums = torch.empty(2, N, dtype=torch.float64, device=x.device)
        fin, fold = _bn_fin(M, N, x.device, bn) if bn is not None else (None, None)
        half = ws[c * nb:(c + 1) * nb]
        e = FwdEpiT(EPI_STATS, col_sums=_p(sums, torch.float64), fin=C.pointer(fin) if fin is not None else None,
                    ws=_p(half, torch.uint8), ws_bytes=half.numel())
        e._keep = (fin, ws)
        descs.append(e)
        extras.append((sums,) if fold is None else (sums, fold))
    _tok = _pb("linear_fwd")
    _call("mmg_linear_fwd_dual", x, _pro(pro0), _pro(pro1), W, bias, outs[0], outs[1], M, N, K, C.byref(descs[0]),
          C.byref(descs[1]), names={"X": "x", "Y0": "out0", "Y1": "out1"})
    _pe(_tok, "linear_fwd", 4 * (M * K + N * K + 2 * M * N), 4 * M * N * K)
    return (outs[0],) + extras[0], (outs[1],) + extras[1]


def linear_wgrad(dy: torch.Tensor, x: torch.Tensor, pro: Optional[Pro] = None, out: Optional[torch.Tensor] = None,
                 accumulate: bool = False, with_bias: bool = False, bias_out: Optional[torch.Tensor] = None,
                 defer: Optional[list] = None):
    """out[N,K] (+)= dy[M,N]^T @ pro(x)[M,K].  with_bias: also return the column sums of dy ([N] float, the bias
    gradient of the same layer), computed in the same pass over dy.
    defer (a list): the partial slabs are NOT summed now -- a job is appended to the list and `out` is complete only after
    wgrad_reduce_flush(list), which sums the slabs of many layers in one launch (nobody reads a weight gradient before the
    optimizer does)."""
    lib = _lib.load()
    M, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise ValueError("linear_wgrad: row mismatch")
    if out is None:
        out = torch.empty(N, K, dtype=torch.float32, device=x.device)
        accumulate = False
    dbias = None
    if with_bias:
        dbias = bias_out if (bias_out is not None and accumulate) else torch.empty(N, dtype=torch.float32, device=x.device)
    nb = lib.mmg_linear_wgrad_ws_bytes(M, N, K)
    _tok = _pb("linear_wgrad")
    if defer is None:
        _call("mmg_linear_wgrad", dy, x, _pro(pro), out, dbias, M, N, K, int(accumulate), ws=nb)
    else:
        if accumulate and lib.mmg_linear_wgrad_is_direct(M, N, K) and any(j[2] is out for j in defer):
            wgrad_reduce_flush(defer)        # a small launch adds into `out` in place: its earlier slabs must be summed first
        ws = torch.empty(max(int(nb), 256), dtype=torch.uint8, device=x.device)      # its own slabs: they live until the flush
        job = WgradReduceT()
        _call("mmg_linear_wgrad_deferred", dy, x, _pro(pro), out, dbias, M, N, K, int(accumulate), C.byref(job), ws=ws)
        defer.append((job, ws, out, dbias))
    _pe(_tok, "linear_wgrad", 4 * (M * N + M * K + N * K), 2 * M * N * K)
    return (out, dbias) if with_bias else out


def wgrad_reduce_flush(jobs: list):
    """Sum the slabs of every deferred weight gradient (linear_wgrad(defer=...)): one launch per <= MMG_WGRAD_REDUCE_MAX
    jobs; a job that accumulates into a gradient an earlier job of the list writes goes into a later launch.  Empties the
    list."""
    if any(len(j) > 4 for j in jobs):        # an entry that lands in a view of a wider matrix: grad_finish places it
        return grad_finish(jobs)
    todo = [j for j in jobs if j[0].slab]
    jobs.clear()
    while todo:
        group, later, seen = [], [], set()
        for j in todo:
            if j[0].dW in seen or len(group) == _lib.MMG_WGRAD_REDUCE_MAX:
                later.append(j)
            else:
                group.append(j)
            seen.add(j[0].dW)            # (also blocks every LATER job of that gradient: the order of its sums is kept)
        arr = (WgradReduceT * len(group))(*[j[0] for j in group])
        _call("mmg_wgrad_reduce_group", arr, len(group))
        todo = later


def _span(t: torch.Tensor):
    """[first byte, one past the last byte) of the storage a tensor's elements lie in (the hull of a strided view)."""
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    last = sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def grad_finish(wjobs: list, sums=()):
    """Everything that finishes the gradients of a step in as few launches as its dependencies allow (mmg_grad_finish_group),
    bit for bit wgrad_reduce_flush(wjobs) followed by vec_sums(sums).  Empties wjobs.
    wjobs: the deferred weight gradients (linear_wgrad(defer=...) entries; a fifth element is the 2-D view the sum lands in
    instead of the entry's `out`, a column slice of a wider matrix).  An accumulating entry on the gradient of an earlier
    one becomes a further slab series of that job.
    sums: (dst, [sources, 1..4]) as vec_sums takes them.  dst is sources[0] = the `out` of an entry: the further sources
    are added by that entry's job, in place.  A sum that reads what a job of the launch writes goes into the next launch."""
    SER = _lib.MMG_GRAD_FINISH_SERIES
    fjs = []                                  # [dst ptr, entry, series [(slab, n_split)], level, dense sources, view]
    last = {}                                 # destination address -> its latest job
    for ent in wjobs:
        job = ent[0]
        if not job.slab:
            continue
        view = ent[4] if len(ent) > 4 else None
        key = view.data_ptr() if view is not None else job.dW
        prev = last.get(key)
        if (prev is not None and job.accumulate and len(prev[2]) < SER and prev[5] is None and view is None and not prev[4]
                and (prev[1][0].n4, prev[1][0].nk4, prev[1][0].dbias) == (job.n4, job.nk4, job.dbias)):
            prev[2].append((job.slab, job.n_split))
            continue
        fj = [key, ent, [(job.slab, job.n_split)], prev[3] + 1 if prev is not None else 0, [], view]
        fjs.append(fj)
        last[key] = fj
    wjobs_keep = list(wjobs)                  # (the slabs live until the launches below are enqueued)
    wjobs.clear()

    def writes(fj):
        ent = fj[1]
        spans = [_span(fj[5] if fj[5] is not None else ent[2])]
        if ent[3] is not None:
            spans.append(_span(ent[3]))
        return spans

    dense = []                                # (dst, sources, level)
    for dst, srcs in sums:
        if not 1 <= len(srcs) <= 4:
            raise ValueError("grad_finish: 1..4 sources per sum")
        if any(t.numel() != dst.numel() for t in srcs):
            raise ValueError("grad_finish: size mismatch")
        host = None
        if dst is srcs[0]:
            host = next((f for f in fjs if f[5] is None and f[1][2] is dst and last[f[0]] is f), None)
        rest = srcs[1:] if host is not None else srcs
        lvl, read = 0, [_span(t) for t in rest]
        for f in fjs:
            if any(a0 < s1 and s0 < a1 for a0, a1 in writes(f) for s0, s1 in read):
                lvl = max(lvl, f[3] + 1)
        ok = (host is not None and lvl <= host[3] and dst.is_contiguous() and dst.numel() == 4 * host[1][0].nk4
              and all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in rest))
        if ok:
            host[4] = list(rest)
        else:
            if host is not None:                       # in place behind the job that writes dst
                lvl = max(lvl, host[3] + 1)
            dense.append((dst, list(srcs), lvl))
    n_lvl = max([f[3] for f in fjs] + [d[2] for d in dense], default=-1) + 1
    for lvl in range(n_lvl):
        group = [f for f in fjs if f[3] == lvl]
        dgroup = [d for d in dense if d[2] == lvl]
        series, sjobs = [], []
        for f in group:
            job, view = f[1][0], f[5]
            series.append(job)
            for slab, n_split in f[2][1:]:               # the accumulating entries that joined it
                series.append(WgradReduceT(slab, job.n4, n_split, job.dW, job.dbias, job.nk4, 1))
            if view is None and not f[4]:
                continue
            # a sum whose first source is the job's dW: the value takes the further sources and lands in the sum's dst
            sp, ld, cols, ld_dst, dst = (C.c_void_p * 4)(), (C.c_int * 4)(), 0, 0, job.dW
            if view is not None:
                if view.dim() != 2 or view.stride(1) != 1 or view.numel() != 4 * job.nk4:
                    raise ValueError("grad_finish: the destination view must be 2-D with unit column stride and the gradient's size")
                cols, ld_dst, dst = view.shape[1], view.stride(0), _p(view, name="", contiguous=False)
            sp[0], ld[0] = job.dW, cols
            for q, sct in enumerate(f[4], 1):
                sp[q], ld[q] = _p(sct, name=""), cols
            sjobs.append(SumJobT(dst, sp, 1 + len(f[4]), 4 * job.nk4, cols, ld_dst, ld))
        for dst, srcs, _ in dgroup:
            views = [_rows_view(x) for x in [dst] + srcs]
            strided = any(c for c, _ in views)
            cols = 0
            if strided:
                if dst.dim() != 2 or any(x.shape != dst.shape for x in srcs):
                    raise ValueError("grad_finish: strided sums take 2-D tensors of one shape")
                cols = dst.shape[1]
            sp, ld = (C.c_void_p * 4)(), (C.c_int * 4)()
            for q, sct in enumerate(srcs):
                sp[q] = _p(sct, name="", contiguous=False)
                ld[q] = (views[q + 1][1] or cols) if strided else 0
            sjobs.append(SumJobT(_p(dst, name="", contiguous=False), sp, len(srcs), dst.numel(), cols,
                                 (views[0][1] or cols) if strided else 0, ld))
        if series or sjobs:
            _call("mmg_grad_finish_group", (WgradReduceT * max(len(series), 1))(*series), len(series),
                  (SumJobT * max(len(sjobs), 1))(*sjobs), len(sjobs))
    del wjobs_keep


def col_reduce2(a: torch.Tensor, b: Optional[torch.Tensor] = None):
    """-> fp64 [2,N]: (sum_m a, sum_m a*b) with b = a when omitted."""
    M, N = a.shape
    out = torch.empty(2, N, dtype=torch.float64, device=a.device)
    _tok = _pb("col_reduce2")
    _call("mmg_col_reduce2", a, b, out, M, N, ws=_lib.load().mmg_col_reduce2_ws_bytes(M, N))
    _pe(_tok, "col_reduce2", 4 * M * N * (2 if b is not None else 1), 0)
    return out


@dataclass
class BNFold:
    scale: torch.Tensor
    shift: torch.Tensor
    mean: torch.Tensor
    rstd: torch.Tensor
    count: int
    training: bool


@dataclass
class NextBN:
    """The BatchNorm backward that CONSUMES an op's output (mmg_next_bn_t): y = its pre-BatchNorm activation, pro = its
    fold / activation / dropout, fold = its BNFold (mean, rstd).  An op that is handed one also returns the fp64 [2,N]
    statistics bn_bwd_stats(out, y, pro, fold) would compute -- from its epilogue where the shape has a fused form, from
    the separate pass elsewhere.  sums: ADD to these sums instead (two producers through one BatchNorm)."""
    y: torch.Tensor
    pro: "Pro"
    fold: "BNFold"
    sums: Optional[torch.Tensor] = None


def _next_bn(nb: NextBN, M: int, N: int):
    """-> (NextBnT for the C call (keeps its prologue alive), the sums tensor the call fills)."""
    lib = _lib.load()
    if tuple(nb.y.shape) != (M, N):
        raise ValueError(f"next_bn: y is {tuple(nb.y.shape)}, the producer writes [{M},{N}]")
    acc = nb.sums is not None
    sums = nb.sums if acc else torch.empty(2, N, dtype=torch.float64, device=nb.y.device)
    if tuple(sums.shape) != (2, N) or sums.dtype != torch.float64:
        raise ValueError("next_bn: sums must be fp64 [2,N]")
    ws = workspace(lib.mmg_epi_ws_bytes(M, N), nb.y.device)
    pc = nb.pro.c()
    t = NextBnT(_p(nb.y), C.pointer(pc), _p(nb.fold.mean), _p(nb.fold.rstd), _p(sums, torch.float64), int(acc),
                _p(ws, torch.uint8), ws.numel())
    t._keep = (pc, ws)
    return t, sums


def bn_finalize(sums: Optional[torch.Tensor], count: int, gamma, beta, running_mean, running_var, training: bool,
                n_updates: int = 1) -> BNFold:
    N = gamma.numel()
    dev = gamma.device
    st = torch.empty(4, N, dtype=torch.float32, device=dev)
    _call("mmg_bn_finalize", sums, count, gamma, beta, running_mean, running_var, int(training), n_updates, BN_MOMENTUM,
          BN_EPS, st[0], st[1], st[2], st[3], N)
    return BNFold(st[0], st[1], st[2], st[3], count, training)


def affine_act_drop(y: torch.Tensor, pro: Pro, out: Optional[torch.Tensor] = None):
    M, N = y.shape
    out = torch.empty_like(y) if out is None else out
    _tok = _pb("affine_act_drop")
    _call("mmg_affine_act_drop", y, _pro(pro), out, M, N)
    _pe(_tok, "affine_act_drop", 8 * M * N, 0)
    return out


def affine_act_drop_rows(y: torch.Tensor, pro: Pro, rows: torch.Tensor):
    """dropout(relu(y[rows]*scale+shift)) for the selected rows (int64 ids); the dropout mask is the one the full tensor
    would get at those rows."""
    N = y.shape[1]
    n = rows.numel()
    out = torch.empty(n, N, dtype=torch.float32, device=y.device)
    _call("mmg_affine_act_drop_rows", y, _pro(pro), rows, n, out, N)
    return out


def bn_bwd_stats(g: torch.Tensor, y: torch.Tensor, pro: Pro, fold: BNFold):
    M, N = y.shape
    out = torch.empty(2, N, dtype=torch.float64, device=y.device)
    _tok = _pb("bn_bwd_stats")
    _call("mmg_bn_bwd_stats", g, y, _pro(pro), fold.mean, fold.rstd, out, M, N,
          ws=_lib.load().mmg_col_reduce2_ws_bytes(M, N))
    _pe(_tok, "bn_bwd_stats", 8 * M * N, 0)
    return out


def bn_bwd_stats2(g: torch.Tensor, g2: torch.Tensor, y: torch.Tensor, pro: Pro, pro2: Pro, fold: BNFold):
    """bn_bwd_stats of two upstream gradients through the same BatchNorm + ReLU with their own dropout masks."""
    M, N = y.shape
    out = torch.empty(2, N, dtype=torch.float64, device=y.device)
    _tok = _pb("bn_bwd_stats")
    _call("mmg_bn_bwd_stats2", g, g2, y, _pro(pro), _pro(pro2), fold.mean, fold.rstd, out, M, N,
          ws=_lib.load().mmg_col_reduce2_ws_bytes(M, N))
    _pe(_tok, "bn_bwd_stats", 12 * M * N, 0)
    return out


def bn_bwd_apply2(g: torch.Tensor, g2: torch.Tensor, y: torch.Tensor, pro: Pro, pro2: Pro, fold: BNFold, sums, count,
                  dbeta=None, dgamma=None):
    M, N = y.shape
    out = torch.empty_like(y)
    _tok = _pb("bn_bwd_apply")
    _call("mmg_bn_bwd_apply2", g, g2, y, _pro(pro), _pro(pro2), fold.mean, fold.rstd, sums, 1.0 / float(count), dbeta,
          dgamma, out, M, N)
    _pe(_tok, "bn_bwd_apply", 16 * M * N, 0)
    return out


def bn_bwd_stats_rows(g_rows: torch.Tensor, y: torch.Tensor, rows: torch.Tensor, pro: Pro, fold: BNFold):
    """bn_bwd_stats for an upstream gradient that is zero outside `rows` (g_rows = its rows, in list order)."""
    N = y.shape[1]
    out = torch.empty(2, N, dtype=torch.float64, device=y.device)
    _call("mmg_bn_bwd_stats_rows", g_rows, y, rows, rows.numel(), _pro(pro), fold.mean, fold.rstd, out, N,
          ws=_lib.load().mmg_bn_bwd_stats_rows_ws_bytes(N))
    return out


def bn_bwd_apply_rows(g_rows: torch.Tensor, y: torch.Tensor, rows: torch.Tensor, pro: Pro, dy: torch.Tensor):
    """dy[rows] += scale * g'  -- completes a bn_bwd_apply(None, ...) for the listed (distinct) rows."""
    _call("mmg_bn_bwd_apply_rows", g_rows, y, rows, rows.numel(), _pro(pro), dy, y.shape[1])
    return dy


def bn_bwd_apply(g: Optional[torch.Tensor], y: torch.Tensor, pro: Pro, fold: Optional[BNFold], sums=None, count: float = 1.0,
                 dbeta=None, dgamma=None, out: Optional[torch.Tensor] = None, accumulate: bool = False):
    """sums: the fp64 [2,N] output of bn_bwd_stats (None in eval mode); dbeta / dgamma ([N] float) receive its rows.
    accumulate: out += (needs out).  g = None: an all-zero upstream gradient (see bn_bwd_apply_rows)."""
    M, N = y.shape
    if accumulate and out is None:
        raise ValueError("accumulate needs out")
    out = torch.empty_like(y) if out is None else out
    _tok = _pb("bn_bwd_apply")
    _call("mmg_bn_bwd_apply", g, y, _pro(pro), fold.mean if fold else None, fold.rstd if fold else None, sums,
          1.0 / float(count), dbeta, dgamma, out, M, N, int(accumulate))
    _pe(_tok, "bn_bwd_apply", (16 if accumulate else 12) * M * N, 0)
    return out


def linear_l2norm_fwd(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None, pro: Optional[Pro] = None):
    """l2norm_fwd(linear_fwd(x, W, bias, pro)) -> (normalised rows, rn): ONE kernel where the GEMM's workgroup holds whole
    rows (the norm is taken in the epilogue, mmg_linear_fwd_supported(MMG_EPI_L2, ...)), the two launches elsewhere."""
    M, K = x.shape
    N = W.shape[0]
    if not _lib.load().mmg_linear_fwd_supported(EPI_L2, M, N, K):
        return l2norm_fwd(linear_fwd(x, W, bias, pro=pro))
    return _linear_fwd(x, W, bias, pro, None, False, False, l2=True)


def linear_fwd_rider_supported(M: int, N: int, K: int, n_sel: int) -> bool:
    return bool(_lib.load().mmg_linear_fwd_rider_supported(int(M), int(N), int(K), int(n_sel)))


@dataclass
class FwdRider:
    """Pairs the compact tail of one pass -- affine_act_drop_rows(y, pro, rows) + linear_l2norm_fwd(act, W, bias) -- with the
    dense linear_l2norm_fwd(x, W, bias, pro=...) of the other pass into ONE launch (mmg_linear_fwd_rider): hand the same
    holder to park_rows and then to linear_l2norm_fwd_rider.  park_rows validates, allocates act / x0 / rn and parks its
    descriptor here WITHOUT launching; the dense call launches both and fills them.  Nothing falls back: a second park on a
    holder that still holds a descriptor, a dense call on an empty holder or with another W or bias raises."""
    parked: Optional[tuple] = None

    def park_rows(self, y: torch.Tensor, pro: Pro, rows: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor]):
        """-> (act, x0, rn) of the listed rows, filled by the dense call that takes this holder."""
        if self.parked is not None:
            raise RuntimeError("FwdRider: the holder already holds a parked tail")
        M, K = y.shape
        N, n = W.shape[0], rows.numel()
        if W.shape[1] != K or not linear_fwd_rider_supported(M, N, K, n):
            raise ValueError(f"FwdRider: no rider for y {tuple(y.shape)}, W {tuple(W.shape)}, {n} rows")
        act = torch.empty(n, K, dtype=torch.float32, device=y.device)
        x0 = torch.empty(n, N, dtype=torch.float32, device=y.device)
        rn = torch.empty(n, dtype=torch.float32, device=y.device)
        self.parked = (y, pro, rows, W, bias, act, x0, rn)
        return act, x0, rn

    def require_consumed(self):
        if self.parked is not None:
            raise RuntimeError("FwdRider: the parked tail was never launched (no dense call followed it)")


def linear_l2norm_fwd_rider(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], pro: Pro, rider: FwdRider):
    """linear_l2norm_fwd(x, W, bias, pro) -> (normalised rows, rn), and in the same launch the tail `rider` parked: its
    act, x0 and rn are bit for bit those of affine_act_drop_rows + linear_l2norm_fwd on the listed rows."""
    if rider.parked is None:
        raise RuntimeError("linear_l2norm_fwd_rider: nothing is parked on the holder")
    y, rpro, rows, rW, rbias, act, x0, rn_a = rider.parked
    same_bias = (bias is None and rbias is None) or (bias is not None and rbias is not None and
                                                     bias.data_ptr() == rbias.data_ptr())
    if W.data_ptr() != rW.data_ptr() or W.shape != rW.shape or not same_bias:
        raise RuntimeError("linear_l2norm_fwd_rider: the parked tail belongs to another W or bias")
    M, K = x.shape
    N = W.shape[0]
    if tuple(y.shape) != (M, K):
        raise ValueError("linear_l2norm_fwd_rider: the parked tail reads a tensor of another shape")
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    rn = torch.empty(M, device=x.device)
    epi = FwdEpiT(EPI_L2, rnorm=_p(rn), eps=L2_EPS)
    epi_a = FwdEpiT(EPI_L2, rnorm=_p(rn_a), eps=L2_EPS)
    _tok = _pb("linear_fwd")
    _call("mmg_linear_fwd_rider", x, _pro(pro), W, bias, out, M, N, K, C.byref(epi), y, _pro(rpro), rows, rows.numel(), W, bias,
          act, x0, C.byref(epi_a), names={"X": "x", "Y": "out", "X_a": "rider.y", "rows": "rider.rows"})
    _pe(_tok, "linear_fwd", 4 * (M * K + N * K + M * N), 2 * M * N * K)
    rider.parked = None
    return out, rn


# mmg_bnbwd_t.mode: linear_bnbwd / _l2bwd / _bnbwd2 / _bnbwd_rows
BNBWD_BN, BNBWD_L2, BNBWD_BN2, BNBWD_ROWS = (_lib.MMG_BNBWD_BN, _lib.MMG_BNBWD_L2, _lib.MMG_BNBWD_BN2,
                                             _lib.MMG_BNBWD_ROWS)


def linear_bnbwd_supported(M: int, N: int, K: int, mode: int = BNBWD_BN, wgrad: bool = False) -> bool:
    return bool(_lib.load().mmg_linear_bnbwd_supported(int(mode), int(M), int(N), int(K), int(wgrad)))


def linear_bnbwd_wgrad_supported(M: int, N: int, K: int) -> bool:
    return linear_bnbwd_supported(M, N, K, wgrad=True)


@dataclass
class FusedWgrad:
    """The weight gradient of the layer whose data gradient a linear_bnbwd / linear_bnbwd2 / linear_bnbwd_rows /
    linear_l2bwd call computes, in the same launch (mmg_bnbwd_wgrad_t): out[K,N] (+)= dz^T @ pro(x), and with with_bias the
    column sums of dz; the arguments mean what they mean for linear_wgrad(dz, x, pro, out, accumulate, with_bias, bias_out,
    defer).  keep_dz=False: dz is not written (the call returns None in its place).  The call fills .dW and .db."""
    x: torch.Tensor
    pro: Optional[Pro] = None
    out: Optional[torch.Tensor] = None
    accumulate: bool = False
    with_bias: bool = False
    bias_out: Optional[torch.Tensor] = None
    defer: Optional[list] = None
    keep_dz: bool = True
    dW: Optional[torch.Tensor] = None
    db: Optional[torch.Tensor] = None


def _fused_wgrad(fw: FusedWgrad, M: int, N: int, K: int):
    """-> BnBwdWgradT for the C call (keeps its prologue, job and workspace alive); sets fw.dW / fw.db."""
    lib = _lib.load()
    if tuple(fw.x.shape) != (M, N):
        raise ValueError(f"fused wgrad: x is {tuple(fw.x.shape)}, expected [{M},{N}]")
    dev = fw.x.device
    acc = fw.accumulate and fw.out is not None
    fw.dW = fw.out if fw.out is not None else torch.empty(K, N, dtype=torch.float32, device=dev)
    fw.db = None
    if fw.with_bias:
        fw.db = fw.bias_out if (fw.bias_out is not None and acc) else torch.empty(K, dtype=torch.float32, device=dev)
    nb = max(int(lib.mmg_linear_bnbwd_wgrad_ws_bytes(M, N, K)), 256)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)      # its own slabs (the shared workspace may hold a NextBN's partials)
    job = WgradReduceT()
    pc = fw.pro.c() if fw.pro is not None else None
    t = BnBwdWgradT(_p(fw.x), C.pointer(pc) if pc is not None else None, _p(fw.dW), _p(fw.db), int(acc),
                    _p(ws, torch.uint8), ws.numel(), C.pointer(job) if fw.defer is not None else None)
    t._keep = (pc, ws, job)
    return t


def _fused_wgrad_done(fw: FusedWgrad, t):
    if fw.defer is not None:
        fw.defer.append((t._keep[2], t._keep[1], fw.dW, fw.db))


def _fused_wgrad_bytes(M: int, N: int, K: int) -> int:      # x read once, one slab per workgroup written
    return 4 * M * N + 4 * int(_lib.load().mmg_linear_bnbwd_wgrad_ws_bytes(M, N, K))


def linear_dgrad_wgrad_supported(M: int, N: int, K: int, p: float = 0.0) -> bool:
    """p: the dropout of the layer input's prologue (the fused launch takes none)."""
    return bool(_lib.load().mmg_linear_dgrad_wgrad_supported(int(M), int(N), int(K), float(p)))


def linear_dgrad_wgrad(dy: torch.Tensor, W: torch.Tensor, wgrad: FusedWgrad, next_bn: Optional["NextBN"] = None):
    """The data gradient and the weight gradient of a plain linear in one launch (mmg_linear_dgrad_wgrad): dx [M,N] =
    dy [M,K] @ W [K,N] (the forward weight, read in place) and wgrad.dW [K,N] (+)= dy^T @ pro(x) -- bit for bit
    linear_fwd(dy, W, w_kn=True) and linear_wgrad(dy, wgrad.x, wgrad.pro, wgrad.out, wgrad.accumulate, defer=wgrad.defer).
    next_bn: + the statistics of the BatchNorm backward that consumes dx, from the epilogue; next_bn.y is wgrad.x and
    next_bn.pro agrees with wgrad.pro.  -> dx, or (dx, sums) with next_bn; the call fills wgrad.dW.  No bias gradient."""
    M, K = dy.shape
    if W.shape[0] != K:
        raise ValueError(f"linear_dgrad_wgrad: W has {W.shape[0]} rows, dy has {K} columns")
    if wgrad.with_bias:
        raise ValueError("linear_dgrad_wgrad: no bias gradient")
    N = W.shape[1]
    dx = torch.empty(M, N, dtype=torch.float32, device=dy.device)
    _tok = _pb("linear_dgrad_wgrad")
    nbt, nsums = _next_bn(next_bn, M, N) if next_bn is not None else (None, None)
    wt = _fused_wgrad(wgrad, M, N, K)
    _call("mmg_linear_dgrad_wgrad", dy, W, dx, M, N, K, C.byref(nbt) if nbt is not None else None, C.byref(wt),
          names={"dY": "dy", "dX": "dx"})
    _fused_wgrad_done(wgrad, wt)
    _pe(_tok, "linear_dgrad_wgrad", 4 * (M * K + K * N + M * N) + _fused_wgrad_bytes(M, N, K), 4 * M * N * K)
    return (dx, nsums) if next_bn is not None else dx


# mode -> (profiler name, [M,K] tensors the kernel reads): g and y; g, g2 and y; y (the listed rows are not counted);
# g and out
_BNBWD_PROF = {BNBWD_BN: ("linear_bnbwd", 2), BNBWD_BN2: ("linear_bnbwd", 3), BNBWD_ROWS: ("linear_bnbwd", 1),
               BNBWD_L2: ("linear_l2bwd", 2)}


@dataclass
class DualBwd:
    """Pairs the masked write of one pass (linear_bnbwd) with the masked accumulate of the other (linear_bnbwd_rows) into ONE
    launch (mmg_linear_bnbwd_dual): hand the same holder to both calls through MaskedDx.pair.  The write validates,
    allocates its outputs, registers its deferred slab job and parks its descriptor here WITHOUT launching; the accumulate
    into the tensor the write returned launches both.  Nothing falls back: a second write on a holder that still holds a
    descriptor, an accumulate on an empty holder or one whose `into` or W is not the parked call's raises."""
    parked: Optional[tuple] = None

    def require_consumed(self):
        if self.parked is not None:
            raise RuntimeError("DualBwd: the parked write was never launched (no accumulate followed it)")


@dataclass
class MaskedDx:
    """The masked dx store of linear_bnbwd / linear_bnbwd_rows (mmg_linear_bnbwd_masked; needs wgrad): dx holds
    dropout(dx) under the mask of `pro` -- which must be the dropout of wgrad.pro -- or, with `into`, that is ADDED to the
    tensor `into` [M,N] (which the call returns as dx).  The consumer of dx applies the activation's select but no dropout.
    pair: the write and the accumulate of the two passes as one launch (see DualBwd; linear_bnbwd_dual_supported)."""
    pro: Pro
    into: Optional[torch.Tensor] = None
    pair: Optional[DualBwd] = None


def linear_bnbwd_dual_supported(M: int, N: int, K: int) -> bool:
    return bool(_lib.load().mmg_linear_bnbwd_dual_supported(int(M), int(N), int(K)))


def linear_bnbwd_masked_supported(M: int, N: int, K: int, mode: int = 0, wgrad: bool = True) -> bool:
    return bool(_lib.load().mmg_linear_bnbwd_masked_supported(int(mode), int(M), int(N), int(K), int(wgrad)))


def _linear_bnbwd(mode: int, y: torch.Tensor, W: torch.Tensor, next_bn: Optional["NextBN"], wgrad: Optional[FusedWgrad],
                  g=None, g2=None, row_pos=None, n_sel=0, pro: Optional[Pro] = None, pro2: Optional[Pro] = None,
                  fold: Optional[BNFold] = None, sums=None, count: float = 1.0, dbeta=None, dgamma=None, rn=None,
                  masked: Optional[MaskedDx] = None):
    """The one call behind linear_bnbwd / linear_bnbwd2 / linear_bnbwd_rows / linear_l2bwd (mmg_linear_bnbwd, or
    mmg_linear_bnbwd_masked with `masked`; the descriptor fields as mmg_bnbwd_t names them).  -> (dz, dx), + the next
    BatchNorm's sums with next_bn."""
    M, K = y.shape
    if W.shape[0] != K:
        raise ValueError(f"{_BNBWD_PROF[mode][0]}: W has {W.shape[0]} rows, y has {K} columns")
    N = W.shape[1]
    if masked is not None:
        if wgrad is None or next_bn is not None:
            raise ValueError(f"{_BNBWD_PROF[mode][0]}: the masked dx store needs wgrad and takes no next_bn")
        if masked.into is not None and (tuple(masked.into.shape) != (M, N) or masked.into.device != y.device):
            raise ValueError(f"{_BNBWD_PROF[mode][0]}: masked.into is {tuple(masked.into.shape)} on {masked.into.device}, "
                             f"expected [{M},{N}] on {y.device}")
    pair = masked.pair if masked is not None else None
    if pair is not None:
        what = f"{_BNBWD_PROF[mode][0]}: the dual launch"
        if mode != (BNBWD_BN if masked.into is None else BNBWD_ROWS):
            raise ValueError(f"{what} pairs a linear_bnbwd write with a linear_bnbwd_rows accumulate")
        if not linear_bnbwd_dual_supported(M, N, K):
            raise ValueError(f"{what} does not cover M={M} N={N} K={K}")
        if masked.into is None:
            pair.require_consumed()
        elif pair.parked is None:
            raise RuntimeError(f"{what}: no parked write to accumulate onto")
        elif pair.parked[0] is not masked.into or pair.parked[1].data_ptr() != W.data_ptr() or pair.parked[1].shape != W.shape:
            raise ValueError(f"{what}: `into` or W is not that of the parked write")
    dz = torch.empty_like(y) if wgrad is None or wgrad.keep_dz else None
    into = masked.into if masked is not None else None
    dx = into if into is not None else torch.empty(M, N, device=y.device)
    name, reads = _BNBWD_PROF[mode]
    nbytes = 4 * (reads * M * K + (M * K if dz is not None else 0) + M * N * (2 if into is not None else 1))
    if wgrad is not None:
        name += "_wgrad"
        nbytes += _fused_wgrad_bytes(M, N, K) + (4 * M if mode == BNBWD_L2 else 0)       # + rn
    elif next_bn is not None:
        nbytes += 4 * M * N                                                              # + the next BatchNorm's y
    _tok = _pb(name)
    nbt, nsums = _next_bn(next_bn, M, N) if next_bn is not None else (None, None)
    wt = _fused_wgrad(wgrad, M, N, K) if wgrad is not None else None
    pcs = [q.c() if q is not None else None for q in (pro, pro2)]          # alive until the call returns
    desc = BnBwdT(mode, _p(g), _p(g2), _p(row_pos, torch.int32), n_sel, _p(y),
                  *[C.pointer(pc) if pc is not None else None for pc in pcs],
                  _p(fold.mean) if fold else None, _p(fold.rstd) if fold else None, _p(sums, torch.float64),
                  1.0 / float(count), _p(dbeta), _p(dgamma), _p(rn), L2_EPS)
    if pair is not None and into is None:
        # parked: the descriptor, what it points into, and the tensors it names stay alive in the holder until the launch
        _fused_wgrad_done(wgrad, wt)               # B's slab series before A's in the finish list
        pair.parked = (dx, W, desc, wt, dz, pcs, (g, y, row_pos, fold, sums, dbeta, dgamma))
        return dz, dx
    if pair is not None:
        _, _, desc_b, wt_b, dz_b, *_keep = pair.parked
        _tok = _pb("linear_bnbwd_dual")
        _call("mmg_linear_bnbwd_dual", C.byref(desc_b), C.byref(wt_b), C.byref(desc), C.byref(wt), W, dz_b, dz, dx, M, N, K)
        pair.parked = None
        _fused_wgrad_done(wgrad, wt)
        nd = (dz is not None) + (dz_b is not None)
        # g and y of the write, y of the accumulate, dx once, x once, two slab series
        _pe(_tok, "linear_bnbwd_dual", 4 * ((3 + nd) * M * K + M * N) + 2 * _fused_wgrad_bytes(M, N, K) - 4 * M * N, 8 * M * N * K)
        return dz, dx
    if masked is not None:
        mpc = masked.pro.c()
        _call("mmg_linear_bnbwd_masked", C.byref(desc), W, dz, dx, M, N, K, C.byref(mpc), int(masked.into is not None),
              C.byref(wt))
    else:
        _call("mmg_linear_bnbwd", C.byref(desc), W, dz, dx, M, N, K, C.byref(nbt) if nbt is not None else None,
              C.byref(wt) if wt is not None else None)
    if wgrad is not None:
        _fused_wgrad_done(wgrad, wt)
    _pe(_tok, name, nbytes, (4 if wgrad is not None else 2) * M * N * K)
    return (dz, dx, nsums) if next_bn is not None else (dz, dx)


def linear_bnbwd(g: torch.Tensor, y: torch.Tensor, pro: Pro, fold: Optional[BNFold], W: torch.Tensor, sums=None,
                 count: float = 1.0, dbeta=None, dgamma=None, next_bn: Optional["NextBN"] = None,
                 wgrad: Optional[FusedWgrad] = None, masked: Optional[MaskedDx] = None):
    """bn_bwd_apply(g, y, ...) and the data gradient dz @ W of the linear in front of that BatchNorm in ONE pass over g and
    y (mmg_linear_bnbwd): -> (dz [M,K], dx [M,N]).  W [K, N] is the forward weight of the linear, read in place.
    next_bn: + the statistics of the BatchNorm backward that consumes dx (see NextBN).
    wgrad: the layer's weight gradient in the same launch (see FusedWgrad).
    masked: dx is stored under, or added under, a dropout mask (see MaskedDx; linear_bnbwd_masked_supported)."""
    return _linear_bnbwd(BNBWD_BN, y, W, next_bn, wgrad, g=g, pro=pro, fold=fold, sums=sums, count=count, dbeta=dbeta,
                         dgamma=dgamma, masked=masked)


def linear_bnbwd2_supported(M: int, N: int, K: int) -> bool:
    return linear_bnbwd_supported(M, N, K, BNBWD_BN2)


def linear_bnbwd2(g: torch.Tensor, g2: torch.Tensor, y: torch.Tensor, pro: Pro, pro2: Pro, fold: BNFold, W: torch.Tensor,
                  sums, count, dbeta=None, dgamma=None, wgrad: Optional[FusedWgrad] = None):
    """bn_bwd_apply2 (two upstream gradients, own dropout masks) + the data gradient dz @ W in one pass -> (dz, dx).
    wgrad: the layer's weight gradient in the same launch (see FusedWgrad)."""
    return _linear_bnbwd(BNBWD_BN2, y, W, None, wgrad, g=g, g2=g2, pro=pro, pro2=pro2, fold=fold, sums=sums, count=count,
                         dbeta=dbeta, dgamma=dgamma)


def linear_bnbwd_rows(g_rows: torch.Tensor, row_pos: torch.Tensor, y: torch.Tensor, pro: Pro, fold: BNFold, W: torch.Tensor,
                      sums, count, dbeta=None, dgamma=None, next_bn: Optional["NextBN"] = None,
                      wgrad: Optional[FusedWgrad] = None, masked: Optional[MaskedDx] = None):
    """bn_bwd_apply(None, ...) + bn_bwd_apply_rows(g_rows, ...) + the data gradient dz @ W in one pass -> (dz, dx): the
    upstream gradient is zero outside the listed rows; row_pos [M] int32 = position of a row in the list or -1.
    next_bn / wgrad / masked: as for linear_bnbwd."""
    return _linear_bnbwd(BNBWD_ROWS, y, W, next_bn, wgrad, g=g_rows if g_rows.numel() else None, row_pos=row_pos,
                         n_sel=g_rows.shape[0], pro=pro, fold=fold, sums=sums, count=count, dbeta=dbeta, dgamma=dgamma,
                         masked=masked)


def linear_bnbwd_rider_supported(M: int, N: int, K: int, n_sel: int) -> bool:
    return bool(_lib.load().mmg_linear_bnbwd_rider_supported(int(M), int(N), int(K), int(n_sel)))


@dataclass
class BwdRider:
    """Pairs the compact L2 backward of one pass -- linear_l2bwd(g_rows, out, rn, W) on its listed rows, and optionally the
    bn_bwd_stats_rows of its dx -- with the dense linear_l2bwd of the other pass into ONE launch (mmg_linear_bnbwd_rider):
    park, then hand the holder to the dense linear_l2bwd.  park validates, allocates dz / dx (/ sums) and parks WITHOUT
    launching; the dense call launches both and fills them.  Nothing falls back: a second park on a holder that still holds a
    descriptor, a dense call on an empty holder, with another W or with a weight gradient raises."""
    parked: Optional[tuple] = None

    def park(self, g_rows: torch.Tensor, out: torch.Tensor, rn: torch.Tensor, W: torch.Tensor, n_rows: int, stats=None):
        """n_rows: the rows of the dense problem.  stats = (y, rows, pro, fold) of bn_bwd_stats_rows(dx, y, rows, pro, fold),
        or None -> (dz, dx, sums or None), filled by the dense call that takes this holder."""
        if self.parked is not None:
            raise RuntimeError("BwdRider: the holder already holds a parked call")
        n, K = out.shape
        N = W.shape[1]
        if W.shape[0] != K or tuple(g_rows.shape) != (n, K) or not linear_bnbwd_rider_supported(n_rows, N, K, n):
            raise ValueError(f"BwdRider: no rider for out {tuple(out.shape)}, W {tuple(W.shape)} beside {n_rows} dense rows")
        dz, dx = torch.empty_like(out), torch.empty(n, N, device=out.device)
        sums = torch.empty(2, N, dtype=torch.float64, device=out.device) if stats is not None else None
        self.parked = (g_rows, out, rn, W, n_rows, stats, dz, dx, sums)
        return dz, dx, sums

    def require_consumed(self):
        if self.parked is not None:
            raise RuntimeError("BwdRider: the parked call was never launched (no dense call followed it)")


def _linear_l2bwd_rider(g, out, rn, W, next_bn, rider: BwdRider):
    """The dense linear_l2bwd and the call parked on `rider` as one launch -> (dz, dx[, the next BatchNorm's sums])."""
    M, K = out.shape
    N = W.shape[1]
    if rider.parked is None:
        raise RuntimeError("linear_l2bwd: nothing is parked on the holder")
    g_a, out_a, rn_a, W_a, n_rows, stats, dz_a, dx_a, sums_a = rider.parked
    if W.data_ptr() != W_a.data_ptr() or W.shape != W_a.shape:
        raise RuntimeError("linear_l2bwd: the parked call belongs to another W")
    if n_rows != M:
        raise ValueError("linear_l2bwd: the parked call was made for a dense problem of another size")
    dz, dx = torch.empty_like(out), torch.empty(M, N, device=out.device)
    nbt, nsums = _next_bn(next_bn, M, N) if next_bn is not None else (None, None)
    desc = BnBwdT(BNBWD_L2, _p(g), None, None, 0, _p(out), None, None, None, None, None, 1.0, None, None, _p(rn), L2_EPS)
    desc_a = BnBwdT(BNBWD_L2, _p(g_a), None, None, 0, _p(out_a), None, None, None, None, None, 1.0, None, None, _p(rn_a), L2_EPS)
    nbt_a = None
    if stats is not None:
        y, rows, pro, fold = stats
        pc = pro.c()
        # (its own buffer: the shared workspace() holds the dense launch's partial rows until the one launch that sums both)
        ws = torch.empty(_lib.load().mmg_bn_bwd_stats_rows_ws_bytes(N), dtype=torch.uint8, device=out.device)
        nbt_a = NextBnT(_p(y), C.pointer(pc), _p(fold.mean), _p(fold.rstd), _p(sums_a, torch.float64), 0, _p(ws, torch.uint8),
                        ws.numel())
    _tok = _pb("linear_l2bwd")
    _call("mmg_linear_bnbwd_rider", C.byref(desc), W, dz, dx, M, N, K, C.byref(nbt) if nbt is not None else None,
          C.byref(desc_a), W, dz_a, dx_a, out_a.shape[0], stats[1] if stats is not None else None,
          C.byref(nbt_a) if nbt_a is not None else None, names={"rows": "rider.rows"})
    _pe(_tok, "linear_l2bwd", 4 * (3 * M * K + M * N * (2 if next_bn is not None else 1)), 2 * M * N * K)
    rider.parked = None
    return (dz, dx, nsums) if next_bn is not None else (dz, dx)


def linear_l2bwd(g: torch.Tensor, out: torch.Tensor, rn: torch.Tensor, W: torch.Tensor, next_bn: Optional["NextBN"] = None,
                 wgrad: Optional[FusedWgrad] = None, rider: Optional[BwdRider] = None):
    """l2norm_bwd(g, out, rn) and the data gradient dz @ W of the linear in front of the normalisation -> (dz, dx): ONE
    kernel where linear_bnbwd_supported (W [K, N] = the forward weight in place), the two launches elsewhere.
    next_bn / wgrad: as for linear_bnbwd (the caller checks linear_bnbwd_wgrad_supported).
    rider: the call parked on this holder rides in the launch (see BwdRider; no wgrad)."""
    M, K = out.shape
    N = W.shape[1]
    if W.shape[0] != K:
        raise ValueError(f"linear_l2bwd: W has {W.shape[0]} rows, out has {K} columns")
    if rider is not None:
        if wgrad is not None:
            raise ValueError("linear_l2bwd: a rider excludes the fused weight gradient")
        return _linear_l2bwd_rider(g, out, rn, W, next_bn, rider)
    if not linear_bnbwd_supported(M, N, K, BNBWD_L2, wgrad is not None):
        if wgrad is not None:
            raise ValueError(f"linear_l2bwd: no fused weight gradient for M={M} N={N} K={K}")
        dz = l2norm_bwd(g, out, rn)
        if next_bn is not None:
            return (dz,) + tuple(linear_fwd(dz, W, w_kn=True, next_bn=next_bn))
        return dz, linear_fwd(dz, W, w_kn=True)
    return _linear_bnbwd(BNBWD_L2, out, W, next_bn, wgrad, g=g, rn=rn)


def l2norm_fwd(z: torch.Tensor):
    M, N = z.shape
    out = torch.empty_like(z)
    rn = torch.empty(M, dtype=torch.float32, device=z.device)
    _tok = _pb("l2norm_fwd")
    _call("mmg_l2norm_fwd", z, out, rn, M, N, L2_EPS)
    _pe(_tok, "l2norm_fwd", 8 * M * N, 0)
    return out, rn


def l2norm_bwd(g: torch.Tensor, out: torch.Tensor, rn: torch.Tensor):
    M, N = out.shape
    dz = torch.empty_like(out)
    _tok = _pb("l2norm_bwd")
    _call("mmg_l2norm_bwd", g, out, rn, dz, M, N, L2_EPS)
    _pe(_tok, "l2norm_bwd", 12 * M * N, 0)
    return dz


def dropout_mask(seed: int, site: int, n_rows: int, width: int, p: float, device, row_offset: int = 0, seed_dev=None):
    """The keep-mask ([n_rows, width] uint8) the kernels draw for (seed, site) -- used to inject the
    same masks into the CPU oracle in parity tests."""
    m = torch.empty(n_rows, width, dtype=torch.uint8, device=device)
    _call("mmg_dropout_mask", seed & 0xFFFFFFFFFFFFFFFF, seed_dev, site, row_offset * width, n_rows * width, float(p), m)
    return m


# ------------------------------------------------------------------------------------------ heads
@dataclass
class Head:
    A: torch.Tensor     # [P,64]
    B: torch.Tensor     # [L,64]
    W2: torch.Tensor    # [32,64]
    b2: torch.Tensor    # [32]
    W3: torch.Tensor    # [32] (mlp.6.weight flattened)
    b3: torch.Tensor    # [1]

    def c(self):
        return HeadT(_p(self.A), _p(self.B), _p(self.W2), _p(self.b2), _p(self.W3), _p(self.b3))


def pair_select(pi, deg, thr: int, dpred=None, io_perm=None, dpred_sorted=None, out=None):
    """Stable compaction of pair positions by head (mmg_pair_select) -> (sel_low, sel_high, counts[2] on device).
    With `dpred`, positions whose upstream gradient is exactly 0 are dropped (dpred is read through io_perm; if
    `dpred_sorted` ([n] float) is given it receives dpred in pair order).  out: the three tensors of an earlier call, to
    be overwritten in place (a captured step holds their addresses)."""
    n = pi.numel()
    if out is not None:
        sel_low, sel_high, counts = out
    else:
        sel_low = torch.empty(max(n, 1), dtype=torch.int32, device=pi.device)
        sel_high = torch.empty(max(n, 1), dtype=torch.int32, device=pi.device)
        counts = torch.empty(2, dtype=torch.int32, device=pi.device)
    _tok = _pb("pair_select")
    _call("mmg_pair_select", pi, deg, thr, dpred, io_perm, dpred_sorted, n, sel_low, sel_high, counts,
          ws=_lib.load().mmg_pair_select_ws_bytes(n))
    _pe(_tok, "pair_select", n * 24)
    return sel_low, sel_high, counts


def _pair_sizes(head: Head, pi, li, deg, pair_id, io_perm, per_pair):
    """The array lengths the kernels range-check against (mmg_pair_head_*: n_total, n_patients, n_labs) must be the real
    ones: every per-pair array has pi's length."""
    n = pi.numel()
    for name, t in (("li", li), ("pair_id", pair_id), ("io_perm", io_perm), ("pred / dpred", per_pair)):
        if t is not None and t.numel() != n:
            raise ValueError(f"pair head: {name} has {t.numel()} entries, pi has {n}")
    if head.A.dim() != 2 or head.A.shape[1] != 64 or head.B.dim() != 2 or head.B.shape[1] != 64:
        raise ValueError("pair head: A and B must be [rows, 64]")


def pair_saved_alloc(n_total: int, device):
    """Buffers of mmg_pair_saved_t: (h1 sign bits int32 [n, 2], layer-2 activations float32 [n, 32]), 136 B per entry.
    n = the pairs of the pair set (entries indexed by pair), or the launch bound of the head's pair list when the entries
    are indexed by list position (by_position).  The forward fills the entries it visits, the backward reads those."""
    return (torch.empty(max(n_total, 1), 2, dtype=torch.int32, device=device),
            torch.empty(max(n_total, 1), 32, dtype=torch.float32, device=device))


def _pair_saved(saved, n_total: int, n_launch: int):
    """saved = (bits, h2) or (bits, h2, by_position): by_position -- entries indexed by the position in the pair list
    instead of the pair index (dense); forward and backward must then run over the same list.  Sizes: one entry per pair
    of the pair set (indexed by pair), or per list position the launch can reach (n_launch, its bound) when by_position."""
    if saved is None:
        return None
    bits, h2 = saved[0], saved[1]
    by_pos = bool(saved[2]) if len(saved) > 2 else False
    need = max(int(n_launch) if by_pos else int(n_total), 1)
    if bits.dtype != torch.int32 or bits.dim() != 2 or bits.shape[1] != 2 or h2.dtype != torch.float32 or h2.dim() != 2 or \
            h2.shape[1] != 32 or bits.shape[0] != h2.shape[0] or not bits.is_contiguous() or not h2.is_contiguous():
        raise ValueError("pair head: saved = (int32 [n, 2], float32 [n, 32]) -- see pair_saved_alloc")
    if bits.shape[0] < need:
        raise ValueError(f"pair head: saved buffers hold {bits.shape[0]} entries, the launch reaches {need}"
                         + (" list positions" if by_pos else " pairs"))
    return PairSavedT(_p(bits, torch.int32), _p(h2), int(by_pos), int(bits.shape[0]))


def pair_head_fwd(head: Head, pi, li, deg, thr: int, want_low: bool, p: float, seed: int, pair_id, pred, seed_dev=None,
                  sel=None, n_sel=None, n_bound: Optional[int] = None, io_perm=None, save=None):
    """sel / n_sel: compacted positions (pair_select) and their device-resident count; n_bound >= that count.
    io_perm: pred is written to pred[io_perm[k]] (the caller's pair order).
    save = pair_saved_alloc(...): also leave what the backward needs per visited pair (mmg_pair_saved_t)."""
    n = pi.numel() if sel is None else int(n_bound)
    if n == 0:
        return
    h = head.c()
    _pair_sizes(head, pi, li, deg, pair_id, io_perm, pred)
    sv = _pair_saved(save, pi.numel(), n)
    _tok = _pb("pair_head_fwd")
    _call("mmg_pair_head_fwd_save", C.byref(h), pi, li, deg, thr, int(want_low), n, pi.numel(),
          min(int(head.A.shape[0]), deg.numel()), int(head.B.shape[0]), float(p), seed & 0xFFFFFFFFFFFFFFFF, seed_dev,
          pair_id, pred, sel, n_sel, io_perm, C.byref(sv) if sv is not None else None)
    _pe(_tok, "pair_head_fwd", n * (12 + (136 if sv is not None else 0)) + 256 * (head.A.shape[0] + head.B.shape[0]),
        n * 2 * (64 * 32 + 32 + 64))


def pair_head_dense_fwd(head: Head, rows, out_rows, out):
    """Every lab of every listed patient row through one head (mmg_pair_head_dense_fwd, inference: no dropout):
    out[out_rows[r], l] = the prediction for (A row rows[r], lab l), l < B.shape[0] -- bitwise what pair_head_fwd returns
    for that pair with p = 0.  rows / out_rows: int32 [n]; out: fp32 [n_out, W] with W >= the number of labs (columns
    beyond it and unlisted rows are left as they are).  Returns out."""
    n = rows.numel()
    if out_rows.numel() != n:
        raise ValueError(f"pair_head_dense_fwd: out_rows has {out_rows.numel()} entries, rows has {n}")
    if head.A.dim() != 2 or head.A.shape[1] != 64 or head.B.dim() != 2 or head.B.shape[1] != 64:
        raise ValueError("pair head: A and B must be [rows, 64]")
    n_labs = int(head.B.shape[0])
    if out.dim() != 2 or out.shape[1] < n_labs:
        raise ValueError(f"pair_head_dense_fwd: out must be [rows, >= {n_labs}], got {list(out.shape)}")
    if n == 0:
        return out
    h = head.c()
    _tok = _pb("pair_head_dense_fwd")
    _call("mmg_pair_head_dense_fwd", C.byref(h), rows, out_rows, n, int(head.A.shape[0]), n_labs, out, int(out.shape[0]),
          int(out.shape[1]))
    _pe(_tok, "pair_head_dense_fwd", n * (8 + 256 + 4 * n_labs) + 256 * n_labs, n * n_labs * 2 * (64 * 32 + 32 + 64))
    return out


def pair_head_bwd(head: Head, grads: Head, pi, li, deg, thr: int, want_low: bool, n_labs: int, p: float, seed: int,
                  pair_id, dpred, seed_dev=None, sel=None, n_sel=None, n_bound: Optional[int] = None, io_perm=None,
                  saved=None):
    """`grads` mirrors `head` (dA,dB,dW2,db2,dW3,db3), accumulated in place.
    saved: what pair_head_fwd(..., save=...) of the SAME head, gate, seed and pair arrays left (it must have visited every
    pair this call visits); None = recompute."""
    n = pi.numel() if sel is None else int(n_bound)
    if n == 0:
        return
    h = head.c()
    g = HeadGradT(_p(grads.A), _p(grads.B), _p(grads.W2), _p(grads.b2), _p(grads.W3), _p(grads.b3))
    _pair_sizes(head, pi, li, deg, pair_id, io_perm, dpred)
    if tuple(grads.A.shape) != tuple(head.A.shape) or tuple(grads.B.shape) != tuple(head.B.shape):
        raise ValueError("pair_head_bwd: gradient tables must have the shapes of A and B")
    sv = _pair_saved(saved, pi.numel(), n)
    _tok = _pb("pair_head_bwd")
    _call("mmg_pair_head_bwd_saved", C.byref(h), C.byref(g), pi, li, deg, thr, int(want_low), n, pi.numel(),
          min(int(head.A.shape[0]), deg.numel()), n_labs, float(p), seed & 0xFFFFFFFFFFFFFFFF, seed_dev, pair_id, dpred,
          sel, n_sel, io_perm, C.byref(sv) if sv is not None else None,
          ws=_lib.load().mmg_pair_head_bwd_ws_bytes(n, n_labs))
    _pe(_tok, "pair_head_bwd", n * 12 + 2 * 256 * (head.A.shape[0] + head.B.shape[0]), n * 2 * (4 * 64 * 32))


# ------------------------------------------------------------------------------------------ loss
LOSS_TYPES = {"mae": 0, "mse": 1, "huber": 2}


def sup_mask_draw(n: int, fraction: float, device, seed: int = 0, seed_dev=None, ids=None, sup=None, count=None,
                  inv_den=None, count_only: bool = False):
    """The per-epoch supervision subset drawn on the device (mmg_sup_mask_draw; train.py:150-176 of the reference)
    -> (sup float [n], count fp64 [1], inv_den fp64 [1] = 1 / max(count, 1)); the three may be passed in (a captured step
    overwrites them in place).  seed_dev: int64 device tensor whose first element is the seed at run time."""
    if count_only:                       # the size of the subset of ids 0 .. n-1, nothing written per pair
        sup = None
    else:
        sup = torch.empty(max(n, 1), dtype=torch.float32, device=device)[:n] if sup is None else sup
    count = torch.empty(1, dtype=torch.float64, device=device) if count is None else count
    inv_den = torch.empty(1, dtype=torch.float64, device=device) if inv_den is None else inv_den
    _call("mmg_sup_mask_draw", seed_dev, int(seed) & 0xFFFFFFFFFFFFFFFF, ids, n, float(fraction), sup if n else None,
          count, inv_den, ws=_lib.load().mmg_sup_mask_ws_bytes(n))
    return sup, count, inv_den


def sup_draw_select(pi, deg, thr: int, fraction: float, seed: int = 0, seed_dev=None, ids=None, io_perm=None, sup=None,
                    out=None, count=None, inv_den=None, max_groups: int = 0, want_sup: bool = True):
    """sup_mask_draw followed by pair_select(pi, deg, thr, sup, io_perm=io_perm) in two launches (mmg_sup_draw_select), bit
    for bit -> (sup float [n] in the caller's order, (sel_low, sel_high, counts), count fp64 [1], inv_den fp64 [1]).
    sup, out, count and inv_den may be passed in (a captured step overwrites them in place); want_sup = False: no mask.
    max_groups > 0: at most that many workgroups."""
    n = pi.numel()
    dev = pi.device
    if not want_sup:
        sup = None
    elif sup is None:
        sup = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    if out is not None:
        sel_low, sel_high, counts = out
    else:
        sel_low = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        sel_high = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.float64, device=dev) if count is None else count
    inv_den = torch.empty(1, dtype=torch.float64, device=dev) if inv_den is None else inv_den
    if sup is not None and sup.numel() != n:
        raise ValueError(f"sup_draw_select: sup has {sup.numel()} entries, pi has {n}")
    for name, t in (("ids", ids), ("io_perm", io_perm)):
        if t is not None and t.numel() != n:
            raise ValueError(f"sup_draw_select: {name} has {t.numel()} entries, pi has {n}")
    _tok = _pb("sup_draw_select")
    _call("mmg_sup_draw_select", seed_dev, int(seed) & 0xFFFFFFFFFFFFFFFF, float(fraction), ids, io_perm, pi, deg, int(thr),
          n, int(max_groups), sup if n else None, sel_low, sel_high, counts, count, inv_den,
          ws=_lib.load().mmg_sup_draw_select_ws_bytes(n))
    _pe(_tok, "sup_draw_select", n * 24)
    return sup, (sel_low, sel_high, counts), count, inv_den


def pair_loss(pred, y, w=None, sup=None, inv_den: float = 1.0, loss_type: str = "mae", inv_den_dev=None, loss_out=None,
              want_dpred: bool = True):
    """-> (loss fp64 scalar tensor, dpred [n]) in one pass (mmg_pair_loss).  inv_den_dev: fp64 [1] device tensor that
    overrides inv_den at run time (a captured step whose supervision subset changes size between replays).
    loss_out: fp64 device scalar to write the loss to (a slot of the caller's buffer); want_dpred = False: loss only."""
    n = pred.numel()
    dpred = torch.empty_like(pred) if want_dpred else None
    loss = torch.empty((), dtype=torch.float64, device=pred.device) if loss_out is None else loss_out
    if loss.numel() != 1:
        raise ValueError("pair_loss: loss_out must hold one fp64 value")
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"Unknown loss type: {loss_type}")            # (model.py:610 of the reference)
    lt = LOSS_TYPES[loss_type]
    _tok = _pb("pair_loss")
    _call("mmg_pair_loss", pred, y, w, sup, n, float(inv_den), inv_den_dev, lt, dpred, loss,
          ws=_lib.load().mmg_pair_loss_ws_bytes(n))
    _pe(_tok, "pair_loss", 20 * n)
    return loss, dpred


class _PairLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, y, w, sup, inv_den, loss_type, inv_den_dev=None):
        loss, dpred = pair_loss(pred.detach().contiguous(), y, w, sup, inv_den, loss_type, inv_den_dev)
        ctx.save_for_backward(dpred)
        return loss.float()

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None, None, None, None


def weighted_pair_loss(pred, y, w=None, sup=None, inv_den: float = 1.0, loss_type: str = "mae", inv_den_dev=None):
    """Differentiable fused loss: inv_den * sum sup*w*|pred-y| (or squared); w/sup are per-pair float vectors."""
    return _PairLossFn.apply(pred, y, w, sup, inv_den, loss_type, inv_den_dev)


# ------------------------------------------------------------------------------------------ evaluation reducers
def seg_sums(pred: torch.Tensor, target: torch.Tensor, seg: torch.Tensor, n_seg: int, n_sigma: float = 0.0,
             want_adjusted: bool = False):
    """Segment sums of the evaluation metrics (mmg_seg_moments + mmg_seg_metrics) -> (sums fp64 [n_seg, 8], adjusted
    predictions or None).  sums[s] = (n, sum|e|, sum e^2, sum t, sum t^2, sum|e/t| over t != 0, count(t != 0), clipped).
    n_sigma > 0: residuals are clipped to mean +- n_sigma * std of their segment first (evaluate.py:417-440)."""
    n = pred.numel()
    dev = pred.device
    nb = _lib.load().mmg_seg_reduce_ws_bytes(n, n_seg)
    moments = None
    if n_sigma > 0:
        moments = torch.empty(n_seg, 3, dtype=torch.float64, device=dev)
        _call("mmg_seg_moments", pred, target, seg, n, n_seg, moments, ws=nb)
    sums = torch.empty(n_seg, 8, dtype=torch.float64, device=dev)
    adj = torch.empty_like(pred) if want_adjusted else None
    _call("mmg_seg_metrics", pred, target, seg, n, n_seg, moments, float(n_sigma), adj, sums, ws=nb)
    return sums, adj


def _rows_view(t: torch.Tensor):
    """(cols, row stride) of a tensor that is a flat vector or a 2-D matrix with unit column stride."""
    if t.is_contiguous():
        return 0, 0
    if t.dim() == 2 and t.stride(1) == 1:
        return t.shape[1], t.stride(0)
    raise ValueError("vec_sums: tensors must be contiguous or 2-D with unit column stride")


def vec_sums(jobs):
    """jobs: list of (dst, [src tensors, 1..4]) -- dst = sum of the sources in list order, ONE launch (mmg_vec_sums).
    2-D tensors may be column slices of wider matrices (row stride > columns): the launch that sums gradient
    contributions also splits / joins the halves of an edge head's first-layer weight."""
    arr = (SumJobT * len(jobs))()
    for j, (dst, srcs) in enumerate(jobs):
        if not 1 <= len(srcs) <= 4:
            raise ValueError("vec_sums: 1..4 sources per job")
        views = [_rows_view(t) for t in [dst] + list(srcs)]
        strided = any(c for c, _ in views)
        cols = 0
        if strided:
            if dst.dim() != 2 or any(t.shape != dst.shape for t in srcs):
                raise ValueError("vec_sums: strided jobs take 2-D tensors of one shape")
            cols = dst.shape[1]
        sp = (C.c_void_p * 4)()
        ld = (C.c_int * 4)()
        for q, t in enumerate(srcs):
            if t.numel() != dst.numel():
                raise ValueError("vec_sums: size mismatch")
            sp[q] = _p(t, name="", contiguous=False)
            ld[q] = (views[q + 1][1] or cols) if strided else 0
        arr[j] = SumJobT(_p(dst, name="", contiguous=False), sp, len(srcs), dst.numel(), cols,
                         (views[0][1] or cols) if strided else 0, ld)
    _call("mmg_vec_sums", arr, len(jobs))


def counters_add(counters, incs):
    """*counters[i] += incs[i] (int64 device scalars) in one launch (mmg_counters_add)."""
    step = _lib.MMG_COUNTERS_MAX
    for i0 in range(0, len(counters), step):
        cs, ins = counters[i0:i0 + step], incs[i0:i0 + step]
        ptrs = (C.c_void_p * len(cs))(*[_p(c, torch.int64) for c in cs])
        inc = (C.c_int64 * len(cs))(*[int(v) for v in ins])
        _call("mmg_counters_add", ptrs, inc, len(cs))


def seed_advance(state: torch.Tensor):
    """state: int64 [2] on the device = (dropout seed the kernels read, stream position); one SplitMix64 step."""
    _call("mmg_seed_advance", state)


def step_advance(adam_steps=(), seed_state: Optional[torch.Tensor] = None, counters=(), incs=()):
    """The one-thread updates that end a captured training step in ONE launch (mmg_step_advance): every optimizer step
    counter += 1 (float device scalars), seed_advance(seed_state), counters_add(counters, incs).  More than one step
    counter, or more than MMG_COUNTERS_MAX counters, take further launches."""
    steps, cmax = list(adam_steps), _lib.MMG_COUNTERS_MAX
    n_calls = max(len(steps), (len(counters) + cmax - 1) // cmax, 1 if seed_state is not None else 0)
    for i in range(n_calls):
        cs, ins = counters[i * cmax:(i + 1) * cmax], incs[i * cmax:(i + 1) * cmax]
        ptrs = (C.c_void_p * max(len(cs), 1))(*[_p(c, torch.int64) for c in cs])
        inc = (C.c_int64 * max(len(cs), 1))(*[int(v) for v in ins])
        _call("mmg_step_advance", steps[i] if i < len(steps) else None, seed_state if i == 0 else None, ptrs, inc, len(cs))


def zeros(*shape, device, dtype=torch.float32):
    """torch.zeros through mmg_fill_zero: a zero-fill KERNEL on the current stream (not hipMemsetAsync -- its hipGraph node
    does not reliably replay the recorded pattern on this ROCm: csrc/common.h, profiles/probes/hipgraph_memset_node.py)."""
    t = torch.empty(*shape, device=device, dtype=dtype)
    _call("mmg_fill_zero", _p(t, dtype), t.numel() * t.element_size())          # void*: any dtype
    return t


# ------------------------------------------------------------------------------------------ grouped small launches
SMALL_MAX_ROWS = 4096


@dataclass
class SmallFwd:
    """One problem of small_fwd_group: out[M,N] (+)= x @ W^T (+ x2 @ W2^T) + bias (w_kn: W, W2 stored [K,N])."""
    x: torch.Tensor
    W: torch.Tensor
    out: Optional[torch.Tensor] = None
    bias: Optional[torch.Tensor] = None
    x2: Optional[torch.Tensor] = None
    W2: Optional[torch.Tensor] = None
    accumulate: bool = False
    w_kn: bool = False


def small_fwd_group(probs: Sequence[SmallFwd], grouped: bool = True):
    """Runs the problems (same N and K) in ceil(len / MMG_SMALL_MAX) launches; allocates missing outputs; returns them.
    grouped False, or a problem with more than SMALL_MAX_ROWS rows: each runs through linear_fwd instead, in list order."""
    if not probs:
        return []
    if not grouped or any(p.x.shape[0] > SMALL_MAX_ROWS for p in probs):
        for p in probs:
            p.out = linear_fwd(p.x, p.W, p.bias, out=p.out, accumulate=p.accumulate, w_kn=p.w_kn)
            if p.x2 is not None:
                linear_fwd(p.x2, p.W2, out=p.out, accumulate=True, w_kn=p.w_kn)
        return [p.out for p in probs]
    K = probs[0].x.shape[1]
    N = probs[0].W.shape[1] if probs[0].w_kn else probs[0].W.shape[0]
    outs = []
    for p in probs:
        M, k = p.x.shape
        n = p.W.shape[1] if p.w_kn else p.W.shape[0]
        if k != K or n != N or (p.W.shape[0] if p.w_kn else p.W.shape[1]) != K or M > SMALL_MAX_ROWS:
            raise ValueError("small_fwd_group: every problem must share (N, K) and have M <= 4096")
        if p.out is None:
            if p.accumulate:
                raise ValueError("accumulate needs out")
            p.out = torch.empty(M, N, dtype=torch.float32, device=p.x.device)
        elif tuple(p.out.shape) != (M, N):
            raise ValueError("small_fwd_group: out shape")
        if (p.x2 is None) != (p.W2 is None) or (p.x2 is not None and (tuple(p.x2.shape) != (M, K) or p.W2.shape != p.W.shape)):
            raise ValueError("small_fwd_group: second term shape")
        outs.append(p.out)
    live = [p for p in probs if p.x.shape[0] > 0]              # (an empty table has an empty output)
    for i0 in range(0, len(live), _lib.MMG_SMALL_MAX):
        chunk = live[i0:i0 + _lib.MMG_SMALL_MAX]
        arr = (SmallFwdT * len(chunk))()
        for i, p in enumerate(chunk):
            arr[i] = SmallFwdT(_p(p.x, name="x"), _p(p.W, name="W"), _p(p.x2), _p(p.W2), _p(p.bias), _p(p.out),
                               p.x.shape[0], _lin_flags(p.accumulate, p.w_kn))
        _call("mmg_small_fwd_group", arr, len(chunk), N, K)
    return outs


@dataclass
class SmallWgrad:
    """One problem of small_wgrad_group: dW[N,K] (+)= dy^T @ x; dbias (+)= column sums of dy (with_bias)."""
    dy: torch.Tensor
    x: torch.Tensor
    dW: Optional[torch.Tensor] = None
    dbias: Optional[torch.Tensor] = None
    with_bias: bool = False
    accumulate: bool = False


def small_wgrad_group(probs: Sequence[SmallWgrad], grouped: bool = True):
    """Runs the problems (same N and K) in ceil(len / MMG_SMALL_MAX) launches; allocates missing outputs; returns [(dW,
    dbias)].  grouped False, or a problem with more than SMALL_MAX_ROWS rows: each runs through linear_wgrad instead."""
    if not probs:
        return []
    if not grouped or any(p.dy.shape[0] > SMALL_MAX_ROWS for p in probs):
        res = [linear_wgrad(p.dy, p.x, out=p.dW, accumulate=p.accumulate, with_bias=p.with_bias, bias_out=p.dbias)
               for p in probs]
        return [r if p.with_bias else (r, None) for p, r in zip(probs, res)]
    N, K = probs[0].dy.shape[1], probs[0].x.shape[1]
    res = []
    for p in probs:
        M = p.dy.shape[0]
        if p.dy.shape[1] != N or p.x.shape[1] != K or p.x.shape[0] != M or M > SMALL_MAX_ROWS:
            raise ValueError("small_wgrad_group: every problem must share (N, K), rows must match, M <= 4096")
        if p.dW is None:
            p.dW = torch.empty(N, K, dtype=torch.float32, device=p.x.device)
            p.accumulate = False
        if p.with_bias and p.dbias is None:
            if p.accumulate:
                raise ValueError("accumulating the bias gradient needs dbias")
            p.dbias = torch.empty(N, dtype=torch.float32, device=p.x.device)
        res.append((p.dW, p.dbias))
    for i0 in range(0, len(probs), _lib.MMG_SMALL_MAX):
        chunk = probs[i0:i0 + _lib.MMG_SMALL_MAX]
        arr = (SmallWgradT * len(chunk))()
        for i, p in enumerate(chunk):
            arr[i] = SmallWgradT(_p(p.dy) if p.dy.numel() else None, _p(p.x) if p.x.numel() else None, _p(p.dW),
                                 _p(p.dbias), p.dy.shape[0], int(p.accumulate))
        _call("mmg_small_wgrad_group", arr, len(chunk), N, K)
    return res


def small_bn_act_group(items, training: bool):
    """items: list of (y [M,N], bn module or None, Pro with the activation / dropout fields) -- the per-type epilogue of
    a HeteroConv layer for every small node type in ONE launch (mmg_small_bn_act_group).
    -> list of (out, BNFold or None); the Pro objects get their scale / shift filled in."""
    res = []
    if not items:
        return res
    N = items[0][0].shape[1]
    for i0 in range(0, len(items), _lib.MMG_SMALL_MAX):
        chunk = items[i0:i0 + _lib.MMG_SMALL_MAX]
        arr = (SmallBnT * len(chunk))()
        keep = []
        for i, (y, mod, pro) in enumerate(chunk):
            M = y.shape[0]
            if y.shape[1] != N or M > SMALL_MAX_ROWS:
                raise ValueError("small_bn_act_group: same width, M <= 4096")
            out = torch.empty_like(y)
            st = torch.empty(4, N, dtype=torch.float32, device=y.device) if mod is not None else None
            arr[i] = SmallBnT(_p(y) if M else None, _p(out) if M else None,
                              _p(mod.weight.detach()) if mod is not None else None,
                              _p(mod.bias.detach()) if mod is not None else None,
                              _p(mod.running_mean) if mod is not None else None,
                              _p(mod.running_var) if mod is not None else None,
                              _p(st), M, int(training), int(pro.relu), float(pro.p),
                              int(pro.seed) & 0xFFFFFFFFFFFFFFFF, int(pro.site), int(pro.row_offset),
                              _p(pro.seed_dev, torch.int64))
            keep.append((out, st))
            fold = None
            if mod is not None:
                fold = BNFold(st[0], st[1], st[2], st[3], M, training)
                pro.scale, pro.shift = st[0], st[1]
            res.append((out, fold))
        _call("mmg_small_bn_act_group", arr, len(chunk), N, BN_MOMENTUM, BN_EPS)
    return res


def small_bn_bwd_group(items):
    """items: list of (g [M,N], y [M,N], Pro, BNFold or None) -> list of (dy, dbeta or None, dgamma or None)
    (mmg_small_bn_bwd_group: the backward of small_bn_act_group, one launch)."""
    res = []
    if not items:
        return res
    N = items[0][1].shape[1]
    for i0 in range(0, len(items), _lib.MMG_SMALL_MAX):
        chunk = items[i0:i0 + _lib.MMG_SMALL_MAX]
        arr = (SmallBnBwdT * len(chunk))()
        for i, (g, y, pro, fold) in enumerate(chunk):
            M = y.shape[0]
            dy = torch.empty_like(y)
            dbg = torch.empty(2, N, dtype=torch.float32, device=y.device) if fold is not None else None
            stats = (fold.scale, fold.shift, fold.mean, fold.rstd, dbg[0], dbg[1]) if fold is not None else (None,) * 6
            arr[i] = SmallBnBwdT(_p(g) if M else None, _p(y) if M else None, _p(dy) if M else None,
                                 *[_p(t) for t in stats], M, int(fold.training) if fold is not None else 0,
                                 int(pro.relu), float(pro.p),
                                 int(pro.seed) & 0xFFFFFFFFFFFFFFFF, int(pro.site), int(pro.row_offset),
                                 _p(pro.seed_dev, torch.int64))
            res.append((dy, dbg[0] if dbg is not None else None, dbg[1] if dbg is not None else None))
        _call("mmg_small_bn_bwd_group", arr, len(chunk), N)
    return res


KNN_WEIGHTS = {"uniform": 0, "distance": 1}


def knn_impute(X, rows, n_neighbors: int, weights: str = "uniform", out=None):
    """sklearn KNNImputer(n_neighbors, weights).fit_transform(X)[rows] over a dense [N, L] fp32 matrix with NaN = missing
    (mmg_knn_impute): observed cells pass through, a missing cell is the (weighted) mean of its lab over the n_neighbors
    nearest rows that observe it (nan-Euclidean distance; ties to the lower row index), a lab nobody has stays NaN.
    rows: int32 [n] receiver rows of X; out: fp32 [n, W >= L] (columns L .. W-1 and the rows of out-of-range receivers are
    left as they are; a new out is NaN there).  Returns out."""
    if weights not in KNN_WEIGHTS:
        raise ValueError(f"knn_impute: weights must be 'uniform' or 'distance', got {weights!r}")
    if X.dim() != 2:
        raise ValueError(f"knn_impute: X must be [rows, labs], got {list(X.shape)}")
    if rows.dim() != 1:
        raise ValueError(f"knn_impute: rows must be 1-D, got {list(rows.shape)}")
    N, L = (int(v) for v in X.shape)
    n = rows.numel()
    if out is None:
        out = torch.full((n, L), float("nan"), dtype=torch.float32, device=X.device)
    elif out.dim() != 2 or out.shape[0] != n or out.shape[1] < L:
        raise ValueError(f"knn_impute: out must be [{n}, >= {L}], got {list(out.shape)}")
    if len({t.device for t in (X, rows, out) if t.is_cuda}) > 1:         # (a host tensor is refused as one, by the call)
        raise ValueError(f"knn_impute: X, rows and out on different devices ({X.device}, {rows.device}, {out.device})")
    _call("mmg_knn_impute", X, N, L, L, rows, n, int(n_neighbors), KNN_WEIGHTS[weights], out, int(out.shape[1]),
          ws=_lib.load().mmg_knn_impute_ws_bytes(N, L, n, int(n_neighbors)))
    return out


# ------------------------------------------------------------------------------------------ leakage audit
MAX_ORDER_RANKS = _lib.MMG_OS_MAX_RANKS
ROBUST_FIELDS = _lib.MMG_RS_FIELDS
SPLIT_FIELDS = _lib.MMG_SM_FIELDS


def order_stats(a: torch.Tensor, ranks: Sequence[int], b: Optional[torch.Tensor] = None, out=None, nan_count=None):
    """Exact order statistics (mmg_order_stats): the values of the 0-based ranks (host ints, at most MAX_ORDER_RANKS) of a -- or of
    |a - b| formed in fp32 -- in ascending order, NaN last.  -> (fp32 [len(ranks)], int64 [1] NaN count), both on the
    device; nothing synchronises with the host."""
    n = a.numel()
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= MAX_ORDER_RANKS:
        raise ValueError(f"order_stats: 1..{MAX_ORDER_RANKS} ranks, got {len(ranks)}")
    if n < 1 or any(r < 0 or r >= n for r in ranks):
        raise ValueError(f"order_stats: ranks {ranks} outside [0, {n})")
    if b is not None and (b.numel() != n or b.device != a.device):
        raise ValueError("order_stats: a and b must have the same length and device")
    if out is None:
        out = torch.empty(len(ranks), dtype=torch.float32, device=a.device)
    if nan_count is None:
        nan_count = torch.empty(1, dtype=torch.int64, device=a.device)
    rk = (C.c_int64 * len(ranks))(*ranks)
    _call("mmg_order_stats", a, b, n, rk, len(ranks), out, nan_count, ws=_lib.load().mmg_order_stats_ws_bytes(n))
    return out, nan_count


def robust_sums(pred: torch.Tensor, target: torch.Tensor, xs: torch.Tensor, nan_count: torch.Tensor, lower, upper, p95,
                out=None):
    """Every sum compute_robust_metrics needs, in one pass (mmg_robust_sums).  xs / nan_count: order_stats of |pred -
    target|; lower / upper / p95: (index into xs of x_i, index of x_j, fp32 gamma) of numpy's "linear" percentile.
    -> fp64 [15] on the device: n, sum|r|, sum r^2, sum t, sum t^2, sum smape term, sum|t|, sum winsorised |r|, sum
    clipped r^2, outside count, NaN count, max|r|, lower, upper, p95 (include/mmgnn.h)."""
    n = pred.numel()
    if n < 1 or target.numel() != n:
        raise ValueError(f"robust_sums: pred and target need the same length >= 1, got {n} and {target.numel()}")
    if not (pred.device == target.device == xs.device == nan_count.device):
        raise ValueError("robust_sums: tensors on different devices")
    if out is None:
        out = torch.empty(ROBUST_FIELDS, dtype=torch.float64, device=pred.device)
    spec = [_lib.PercentileT(int(lo), int(hi), float(g)) for lo, hi, g in (lower, upper, p95)]
    _call("mmg_robust_sums", pred, target, n, xs, xs.numel(), nan_count, *spec, out,
          ws=_lib.load().mmg_robust_sums_ws_bytes(n))
    return out


def split_membership(patient: torch.Tensor, train_mask: torch.Tensor, val_mask: torch.Tensor, test_mask: torch.Tensor,
                     n_patients: int, out=None):
    """Patients per split-membership class (mmg_split_membership).  patient: int64 [E]; masks: bool [E].
    -> int64 [10] on the device: [m] for m = 1..7 the patients whose edges fall in exactly the splits of bit mask m
    (1 train, 2 val, 4 test), [8] edges in more than one split, [9] edges in train and in val or test."""
    E = patient.numel()
    masks = (train_mask, val_mask, test_mask)
    if any(m.numel() != E for m in masks):
        raise ValueError("split_membership: every mask needs one entry per edge")
    if any(m.device != patient.device for m in masks):
        raise ValueError("split_membership: tensors on different devices")
    if out is None:
        out = torch.empty(SPLIT_FIELDS, dtype=torch.int64, device=patient.device)
    _call("mmg_split_membership", patient, *masks, E, int(n_patients), out,
          names={"train_mask": "mask", "val_mask": "mask", "test_mask": "mask", "counts": "out"},
          ws=_lib.load().mmg_split_membership_ws_bytes(int(n_patients)))
    return out


# ------------------------------------------------------------------------------------------ lab preprocessing
PREP_MAX_LABS = _lib.MMG_PREP_MAX_LABS
LAB_STAT_FIELDS = _lib.MMG_LS_FIELDS          # n, mean, std, min, max, q25, median, q75, rows
LS_N, LS_MEAN, LS_STD, LS_MIN, LS_MAX, LS_Q25, LS_MEDIAN, LS_Q75, LS_ROWS = (
    _lib.MMG_LS_N, _lib.MMG_LS_MEAN, _lib.MMG_LS_STD, _lib.MMG_LS_MIN, _lib.MMG_LS_MAX, _lib.MMG_LS_Q25, _lib.MMG_LS_MEDIAN,
    _lib.MMG_LS_Q75, _lib.MMG_LS_ROWS)
SORT_BY_TIME, SORT_BY_VALUE = _lib.MMG_PS_TIME, _lib.MMG_PS_VALUE
AGG_CODES = {"last": _lib.MMG_AGG_LAST, "mean": _lib.MMG_AGG_MEAN, "median": _lib.MMG_AGG_MEDIAN, "min": _lib.MMG_AGG_MIN,
             "max": _lib.MMG_AGG_MAX}
OUTLIER_CODES = {None: _lib.MMG_OUT_NONE, "std": _lib.MMG_OUT_STD, "iqr": _lib.MMG_OUT_IQR}
NORM_CODES = {"zscore": _lib.MMG_NORM_ZSCORE, "minmax": _lib.MMG_NORM_MINMAX, "robust": _lib.MMG_NORM_ROBUST}
_LT_OUTLIER, _LT_NORMALIZE, _LT_INVERSE = _lib.MMG_LT_OUTLIER, _lib.MMG_LT_NORMALIZE, _lib.MMG_LT_INVERSE


def _prep_sizes(n, n_patients, n_labs):
    if not (0 <= n < 2 ** 31 - 1 and 1 <= n_patients < 2 ** 31 - 1 and 1 <= n_labs <= PREP_MAX_LABS):
        raise ValueError(f"lab preprocessing: n {n}, n_patients {n_patients}, n_labs {n_labs} outside [0, 2^31) / "
                         f"[1, 2^31) / [1, {PREP_MAX_LABS}]")


def prep_sort(lab: torch.Tensor, patient: Optional[torch.Tensor], secondary: Optional[torch.Tensor], n_patients: int,
              n_labs: int, value: Optional[torch.Tensor] = None):
    """Stable sort of the rows by (lab * n_patients + patient, secondary) (mmg_prep_sort).  secondary: int64 times
    (INT64_MAX = missing, last), fp64 values (NaN last) or None.  -> (perm int32 [n], group int64 [n] at the sorted
    positions, value[perm] or None); rows with a code out of range come last under the group n_labs * n_patients."""
    n = lab.numel()
    n_patients = int(n_patients) if patient is not None else 1
    _prep_sizes(n, n_patients, n_labs)
    kind = SORT_BY_VALUE if secondary is not None and secondary.dtype == torch.float64 else SORT_BY_TIME
    if secondary is not None and secondary.numel() != n:
        raise ValueError("prep_sort: secondary needs one entry per row")
    if (patient is not None and patient.numel() != n) or (value is not None and value.numel() != n):
        raise ValueError("prep_sort: every column needs one entry per row")
    perm = torch.empty(n, dtype=torch.int32, device=lab.device)
    group = torch.empty(n, dtype=torch.int64, device=lab.device)
    vs = torch.empty(n, dtype=torch.float64, device=lab.device) if value is not None else None
    # secondary is void*: int64 times or fp64 values, as `kind` says
    _call("mmg_prep_sort", lab, patient, _p(secondary, torch.float64 if kind == SORT_BY_VALUE else torch.int64, "secondary"),
          kind, n, n_patients, int(n_labs), value, perm, group, vs, names={"value_src": "value"},
          ws=_lib.load().mmg_prep_sort_ws_bytes(n))
    return perm, group, vs


_SORTED_NAMES = {"group_sorted": "group", "value_sorted": "value"}       # what the refusals of these wrappers call them


def lab_stats(group_sorted: torch.Tensor, value_sorted: torch.Tensor, n_patients: int, n_labs: int, out=None):
    """Per-lab n / mean / std (ddof 1) / min / max / rows over a lab-sorted array (mmg_lab_stats) -> fp64
    [n_labs, 9] on the device, the quantile fields NaN."""
    n = value_sorted.numel()
    _prep_sizes(n, n_patients, n_labs)
    if group_sorted.numel() != n:
        raise ValueError("lab_stats: group and value need the same length")
    if out is None:
        out = torch.empty(n_labs, LAB_STAT_FIELDS, dtype=torch.float64, device=value_sorted.device)
    _call("mmg_lab_stats", group_sorted, value_sorted, n, int(n_patients), int(n_labs), out, names=_SORTED_NAMES,
          ws=_lib.load().mmg_lab_stats_ws_bytes(n_labs))
    return out


def lab_quantiles(group_sorted: torch.Tensor, value_sorted: torch.Tensor, n_patients: int, n_labs: int,
                  stats: torch.Tensor):
    """q25 / median / q75 of every lab from a (lab, value)-sorted array into stats (mmg_lab_quantiles)."""
    n = value_sorted.numel()
    _prep_sizes(n, n_patients, n_labs)
    if group_sorted.numel() != n or tuple(stats.shape) != (n_labs, LAB_STAT_FIELDS):
        raise ValueError("lab_quantiles: group / value lengths or the stats shape do not match")
    _call("mmg_lab_quantiles", group_sorted, value_sorted, n, int(n_patients), int(n_labs), stats, names=_SORTED_NAMES,
          ws=_lib.load().mmg_lab_quantiles_ws_bytes(n_labs))
    return stats


def lab_aggregate(group_sorted: torch.Tensor, value_sorted: torch.Tensor, n_patients: int, n_labs: int, method: str,
                  outlier_method: Optional[str] = None, threshold: float = 5.0, stats: Optional[torch.Tensor] = None):
    """One value per (patient, lab) segment of the sorted events (mmg_lab_aggregate) -> (patient, lab, value) in (lab,
    patient) order.  Waits for the stream: the pair count comes back to size the results."""
    n = value_sorted.numel()
    _prep_sizes(n, n_patients, n_labs)
    if group_sorted.numel() != n:
        raise ValueError("lab_aggregate: group and value need the same length")
    dev = value_sorted.device
    op = torch.empty(n, dtype=torch.int64, device=dev)
    ol = torch.empty(n, dtype=torch.int64, device=dev)
    ov = torch.empty(n, dtype=torch.float64, device=dev)
    cnt = C.c_int64(0)
    _call("mmg_lab_aggregate", group_sorted, value_sorted, n, int(n_patients), int(n_labs), AGG_CODES[method],
          OUTLIER_CODES[outlier_method], float(threshold), stats, op, ol, ov, C.byref(cnt), names=_SORTED_NAMES,
          ws=_lib.load().mmg_lab_aggregate_ws_bytes(n))
    k = int(cnt.value)
    return op[:k], ol[:k], ov[:k]


def lab_transform(mode: int, method: int, value: torch.Tensor, lab: Optional[torch.Tensor], stats: torch.Tensor,
                  threshold: float = 0.0, out=None):
    """Element-wise outlier masking / normalise / inverse over the per-lab table (mmg_lab_transform), fp64."""
    n = value.numel()
    n_labs = stats.shape[0]
    if stats.dim() != 2 or stats.shape[1] != LAB_STAT_FIELDS or (lab is not None and lab.numel() != n):
        raise ValueError("lab_transform: stats must be [n_labs, 9] and lab as long as value")
    if out is None:
        out = torch.empty_like(value)
    _call("mmg_lab_transform", mode, method, float(threshold), lab, value, n, int(n_labs), stats, out)
    return out


def lab_outlier_mask(value, lab, stats, method: str, threshold: float):
    return lab_transform(_LT_OUTLIER, OUTLIER_CODES[method], value, lab, stats, threshold)


def lab_normalize(value, lab, stats, method: str):
    return lab_transform(_LT_NORMALIZE, NORM_CODES[method], value, lab, stats)


def lab_inverse(value, lab, stats, method: str):
    return lab_transform(_LT_INVERSE, NORM_CODES[method], value, lab, stats)


def lab_inverse_matrix(pred: torch.Tensor, stats: torch.Tensor, method: str, out=None):
    """The inverse normalisation of a dense fp32 [n_rows, n_labs] matrix (rows may be strided) (mmg_lab_inverse_matrix)."""
    if pred.dim() != 2 or pred.stride(1) != 1 or pred.shape[1] != stats.shape[0] or stats.shape[1] != LAB_STAT_FIELDS:
        raise ValueError("lab_inverse_matrix: pred must be [n_rows, n_labs] with unit column stride, stats [n_labs, 9]")
    pp = _p(pred, torch.float32, "pred", contiguous=False)
    if out is None:
        out = torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
    _call("mmg_lab_inverse_matrix", NORM_CODES[method], pp, pred.shape[0], pred.shape[1],
          pred.stride(0) if pred.shape[0] > 1 else max(pred.stride(0), pred.shape[1]), stats, out, out.shape[1])
    return out


# ------------------------------------------------------------------------------------------ feature-space selection
SEL_ROWS = {"all": _lib.MMG_SEL_ROWS_ALL, "first": _lib.MMG_SEL_ROWS_FIRST}


def code_select(code: torch.Tensor, patient: torch.Tensor, n_patients: int, n_codes: int, min_patient_count: int,
                top_k: Optional[int] = None, rows: str = "all", valid: Optional[torch.Tensor] = None):
    """Per-code patient and row counts, the rank of the eligible codes, the selected codes and the kept rows
    (mmg_code_select).  code, patient: int64 device tensors over the rows (out of range = the row is ignored); valid:
    uint8 / bool or None.  -> (n_patients_per_code int64 [n_codes], n_rows_per_code int64 [n_codes], rank int32
    [n_codes], selected uint8 [n_codes], out_rows int32, ascending).  Waits for the stream: the row count comes back."""
    n = code.numel()
    if rows not in SEL_ROWS:
        raise ValueError(f'code_select: rows must be "all" or "first", got {rows!r}')
    if not (0 <= n < 2 ** 31 - 1 and 1 <= n_patients < 2 ** 31 - 1 and 1 <= n_codes < 2 ** 31 - 1):
        raise ValueError(f"code_select: n {n}, n_patients {n_patients}, n_codes {n_codes} outside [0, 2^31) / [1, 2^31) / "
                         f"[1, 2^31)")
    if patient.numel() != n or (valid is not None and valid.numel() != n):
        raise ValueError("code_select: every column needs one entry per row")
    dev = code.device
    n_pat = torch.empty(n_codes, dtype=torch.int64, device=dev)
    n_rows = torch.empty(n_codes, dtype=torch.int64, device=dev)
    rank = torch.empty(n_codes, dtype=torch.int32, device=dev)
    selected = torch.empty(n_codes, dtype=torch.uint8, device=dev)
    out_rows = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = C.c_int64(0)
    _call("mmg_code_select", code, patient, valid, n, int(n_patients), int(n_codes), int(min_patient_count),
          -1 if top_k is None else int(top_k), SEL_ROWS[rows], n_pat, n_rows, rank, selected, out_rows, C.byref(cnt),
          ws=_lib.load().mmg_code_select_ws_bytes(n, int(n_codes)))
    return n_pat, n_rows, rank, selected, out_rows[:int(cnt.value)]


# ------------------------------------------------------------------------------------------ device graph build
def first_seen_index(code: torch.Tensor, n_codes: int, valid: Optional[torch.Tensor] = None):
    """Node indices in first-seen order (mmg_first_seen_index).  code: int64 device tensor over the rows (out of range =
    the row is ignored); valid: uint8 / bool or None.  -> (index_of_code int32 [n_codes], -1 = never seen;
    code_of_index int64 [number of codes seen]).  Waits for the stream: the count comes back."""
    n = code.numel()
    if not (0 <= n < 2 ** 31 - 1 and 1 <= n_codes < 2 ** 31 - 1):
        raise ValueError(f"first_seen_index: n {n}, n_codes {n_codes} outside [0, 2^31) / [1, 2^31)")
    if valid is not None and valid.numel() != n:
        raise ValueError("first_seen_index: every column needs one entry per row")
    dev = code.device
    index_of_code = torch.empty(n_codes, dtype=torch.int32, device=dev)
    code_of_index = torch.empty(min(n, int(n_codes)), dtype=torch.int64, device=dev)
    cnt = C.c_int64(0)
    _call("mmg_first_seen_index", code, valid, n, int(n_codes), index_of_code, code_of_index, C.byref(cnt),
          ws=_lib.load().mmg_first_seen_index_ws_bytes(n, int(n_codes)))
    return index_of_code, code_of_index[:int(cnt.value)]


def edge_build(patient: torch.Tensor, item: torch.Tensor, patient_index: torch.Tensor, item_index: torch.Tensor,
               value: Optional[torch.Tensor] = None, reverse: bool = True):
    """One edge per row whose two codes have an index, row order kept (mmg_edge_build).  patient, item: int64 device
    tensors over the rows; patient_index, item_index: the int32 tables of first_seen_index; value: fp64 or None.
    -> (fwd int64 [2, E] contiguous, rev = fwd.flip(0) or None, attr fp32 [E] or None).  Waits for the stream: E comes
    back.  The kernels write into [2, n] buffers; when rows were dropped (E < n) the [2, E] result is their narrowing
    copy."""
    n = patient.numel()
    if not 0 <= n < 2 ** 31 - 1:
        raise ValueError(f"edge_build: n {n} outside [0, 2^31)")
    if item.numel() != n or (value is not None and value.numel() != n):
        raise ValueError("edge_build: every column needs one entry per row")
    dev = patient.device
    fwd = torch.empty((2, n), dtype=torch.int64, device=dev)
    rev = torch.empty((2, n), dtype=torch.int64, device=dev) if reverse else None
    attr = torch.empty(n, dtype=torch.float32, device=dev) if value is not None else None
    cnt = C.c_int64(0)
    _call("mmg_edge_build", patient, item, value, n, patient_index, patient_index.numel(), item_index,
          item_index.numel(), fwd, rev, n, attr, C.byref(cnt), ws=_lib.load().mmg_edge_build_ws_bytes(n))
    E = int(cnt.value)
    if E < n:
        fwd = fwd[:, :E].contiguous()
        rev = rev[:, :E].contiguous() if reverse else None
        attr = attr[:E] if attr is not None else None
    return fwd, rev, attr


# ------------------------------------------------------------------------------------------ prediction analysis
AN_MAX_LABS = 2048          # the lab limit of csrc/analysis.hip (and of csrc/evalred.hip)
AN_MAX_BINS = _lib.MMG_AN_MAX_BINS
AN_LAB_FIELDS = _lib.MMG_AN_LAB_FIELDS      # n, sum t, sum p, sum t^2, sum t p, sum |p - t|, sum (p - t)^2, min t, max t
AN_BIN_FIELDS = _lib.MMG_AN_BIN_FIELDS      # n, sum |p - t|


def _an_index(t: Optional[torch.Tensor], n: int, name: str, dev):
    if t is None:
        return None, 8
    if t.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"{name}: expected int64 or int32 indices, got {t.dtype}")
    if t.numel() != n:
        raise ValueError(f"{name}: {t.numel()} indices for {n} pairs")
    if t.device != dev:
        raise ValueError(f"{name}: tensors on different devices")
    return _p(t, t.dtype, name), t.element_size()


def _an_args(what, pred, target, patient, lab, n_labs, deg, bin_edges):
    n = target.numel()
    dev = target.device
    if pred is not None and (pred.numel() != n or pred.device != dev):
        raise ValueError(f"{what}: pred and target need the same length and device")
    pl, ib_l = _an_index(lab, n, "lab", dev)
    pp, ib_p = _an_index(patient, n, "patient", dev)
    if lab is not None and patient is not None and ib_l != ib_p:
        raise TypeError(f"{what}: patient and lab indices must have the same dtype")
    n_labs = int(n_labs) if lab is not None else 0
    edges = [float(e) for e in bin_edges] if (bin_edges is not None and patient is not None) else []
    n_bins = max(len(edges) - 1, 0)
    if n_bins and deg is None:
        raise ValueError(f"{what}: degree bins need deg")
    ed = (C.c_double * (n_bins + 1))(*edges) if n_bins else None
    ib = ib_l if lab is not None else ib_p
    return n, dev, pl, pp, ib, n_labs, n_bins, ed


def pair_analysis(pred: torch.Tensor, target: torch.Tensor, lab: Optional[torch.Tensor] = None, n_labs: int = 0,
                  patient: Optional[torch.Tensor] = None, deg: Optional[torch.Tensor] = None, bin_edges=None):
    """One read of the pairs (mmg_pair_analysis) -> (lab_sums fp64 [n_labs, 9] or None, bin_sums fp64 [n_bins, 2] or
    None), on the device.  lab / patient: int64 or int32 [n]; deg: int32 [n_patients]; bin_edges: ascending host floats,
    bin j = [edges[j], edges[j + 1]).  Fixed-order fp64 sums: bitwise reproducible; nothing synchronises with the host."""
    n, dev, pl, pp, ib, n_labs, n_bins, ed = _an_args("pair_analysis", pred, target, patient, lab, n_labs, deg, bin_edges)
    lab_sums = torch.empty(n_labs, AN_LAB_FIELDS, dtype=torch.float64, device=dev) if n_labs else None
    bin_sums = torch.empty(n_bins, AN_BIN_FIELDS, dtype=torch.float64, device=dev) if n_bins else None
    _call("mmg_pair_analysis", pred, target, pp if n_bins else None, pl, ib, n, n_labs, deg if n_bins else None,
          deg.numel() if n_bins else 0, ed, n_bins, lab_sums, bin_sums,
          ws=_lib.load().mmg_pair_analysis_ws_bytes(n, n_labs, n_bins))
    return lab_sums, bin_sums


def pair_calibrated_abs(pred: Optional[torch.Tensor], target: torch.Tensor, lab: Optional[torch.Tensor] = None,
                        a: Optional[torch.Tensor] = None, b: Optional[torch.Tensor] = None,
                        patient: Optional[torch.Tensor] = None, deg: Optional[torch.Tensor] = None, bin_edges=None,
                        bin_mean: Optional[torch.Tensor] = None):
    """The second read (mmg_pair_calibrated_abs) -> (lab_abs fp64 [n_labs] = sum |(a t + b) - t| with fp32 a, b [n_labs],
    or None; bin_sq fp64 [n_bins] = sum (|p - t| - bin_mean)^2, or None), on the device."""
    n, dev, pl, pp, ib, n_labs, n_bins, ed = _an_args("pair_calibrated_abs", pred, target, patient, lab,
                                                      a.numel() if a is not None else 0, deg, bin_edges)
    if n_labs and (b is None or b.numel() != n_labs):
        raise ValueError("pair_calibrated_abs: a and b need one entry per lab")
    if n_bins and (bin_mean is None or bin_mean.numel() != n_bins or pred is None):
        raise ValueError("pair_calibrated_abs: degree bins need pred and one mean per bin")
    lab_abs = torch.empty(n_labs, dtype=torch.float64, device=dev) if n_labs else None
    bin_sq = torch.empty(n_bins, dtype=torch.float64, device=dev) if n_bins else None
    _call("mmg_pair_calibrated_abs", pred if n_bins else None, target, pp if n_bins else None, pl, ib, n, n_labs,
          a if n_labs else None, b if n_labs else None, deg if n_bins else None, deg.numel() if n_bins else 0, ed, n_bins,
          bin_mean if n_bins else None, lab_abs, bin_sq, ws=_lib.load().mmg_pair_calibrated_abs_ws_bytes(n, n_labs, n_bins))
    return lab_abs, bin_sq


# ------------------------------------------------------------------------------------------ embedding maps
PCA_MAX_D = 256              # the widest X of csrc/pca.hip; D is a multiple of 4 in [4, PCA_MAX_D]
PCA_MAX_K = 8                # components per mmg_project_rows call
GRID_MAX = 256               # cells per axis of mmg_grid2d


def _rows_matrix(x: torch.Tensor, name: str):
    """fp32 device [n, D] with unit column stride -> (pointer, n, D, row stride in elements)."""
    if x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError(f"{name}: expected a 2-D tensor with unit column stride")
    px = _p(x, torch.float32, name, contiguous=False)
    n, D = int(x.shape[0]), int(x.shape[1])
    ld = int(x.stride(0)) if n > 1 else max(int(x.stride(0)), D)
    return px, n, D, ld


def _lab_matrix(X: torch.Tensor, what: str):
    """An fp32 [patients, labs] matrix whose rows may be strided -> (pointer, n, L, row stride)."""
    if not torch.is_tensor(X) or X.dim() != 2:
        raise ValueError(f"{what}: X must be a 2-D tensor [patients, labs]")
    return _rows_matrix(X, "X")


def slab_plan(binding, symbol: str, n: int, n_labs: int):
    """The slab plan of a satellite's fp64 Gram kernel (csrc/gram64.h) from its host function `symbol`
    -> (rows per slab, slabs)."""
    rows, slabs = C.c_int64(0), C.c_int(0)
    check(getattr(binding.load(), symbol)(int(n), int(n_labs), C.byref(rows), C.byref(slabs)), symbol)
    return int(rows.value), int(slabs.value)


def centered_gram(x: torch.Tensor):
    """Column means and the centred Gram matrix of fp32 [n, D] rows (mmg_centered_gram) -> (mean fp64 [D], S fp64
    [D, D] = sum_i (x_i - mean)(x_i - mean)^T, exactly symmetric), on the device.  Fixed-order fp64 sums: bitwise
    reproducible; nothing synchronises with the host."""
    px, n, D, ld = _rows_matrix(x, "x")
    mean = torch.empty(D, dtype=torch.float64, device=x.device)
    gram = torch.empty(D, D, dtype=torch.float64, device=x.device)
    _call("mmg_centered_gram", px, n, D, ld, mean, gram, ws=_lib.load().mmg_centered_gram_ws_bytes(n, D))
    return mean, gram


def project_rows(x: torch.Tensor, mean: torch.Tensor, comps: torch.Tensor, scale: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None):
    """out[i, c] = scale[c] * sum_d (x[i, d] - mean[d]) * comps[c, d] (mmg_project_rows): fp64 sums rounded once to
    fp32 [n, k].  mean fp64 [D], comps fp64 [k, D], scale fp64 [k] or None, all on the device."""
    px, n, D, ld = _rows_matrix(x, "x")
    if comps.dim() != 2 or comps.shape[1] != D or mean.numel() != D:
        raise ValueError(f"project_rows: comps must be [k, {D}] and mean [{D}]")
    k = int(comps.shape[0])
    if scale is not None and scale.numel() != k:
        raise ValueError(f"project_rows: scale needs one entry per component ({k})")
    if out is None:
        out = torch.empty(n, k, dtype=torch.float32, device=x.device)
    elif out.shape != (n, k):
        raise ValueError(f"project_rows: out must be [{n}, {k}]")
    _call("mmg_project_rows", px, n, D, ld, mean, comps, scale, k, out, k)          # takes no workspace: ws = NULL
    return out


def grid2d(y: torch.Tensor, ex: torch.Tensor, ey: torch.Tensor, w: Optional[torch.Tensor] = None):
    """numpy.histogram2d of the fp32 points y [n, 2] over explicit fp64 device edges ex [gx + 1], ey [gy + 1]
    (mmg_grid2d) -> (count int64 [gx, gy], wsum int64 [gx, gy] = the sum of the int32 weights w per cell, or None)."""
    if y.dim() != 2 or y.shape[1] < 2:
        raise ValueError("grid2d: y must be [n, >= 2]")
    py, n, _, ld = _rows_matrix(y, "y")
    gx, gy = int(ex.numel()) - 1, int(ey.numel()) - 1
    if w is not None and w.numel() != n:
        raise ValueError(f"grid2d: {w.numel()} weights for {n} points")
    count = torch.empty(max(gx, 0), max(gy, 0), dtype=torch.int64, device=y.device)
    wsum = torch.empty_like(count) if w is not None else None
    _call("mmg_grid2d", py, max(ld, 2), w, n, ex, ey, gx, gy, count, wsum)          # takes no workspace: ws = NULL
    return count, wsum


# ------------------------------------------------------------------------------------------ exact t-SNE
TSNE_MAX_N = _lib.MMG_TSNE_MAX_N                   # csrc/tsne.hip: 4 <= n <= TSNE_MAX_N
TSNE_TILE = _lib.MMG_TSNE_TILE                     # points of Y per LDS tile of the step kernels
TSNE_SEARCH_WIDTH = _lib.MMG_TSNE_SEARCH_WIDTH     # threads that reduce one row of the perplexity search


def _tsne_square(a: torch.Tensor, name: str):
    """The fp32 device n x n buffer of the t-SNE calls (unit column stride; the rows may be padded) -> (pointer, n, ld)."""
    pa, n, m, ld = _rows_matrix(a, name)
    if n != m:
        raise ValueError(f"{name}: expected a square [n, n] buffer, got [{n}, {m}]")
    return pa, n, ld


def tsne_sqdist(x: torch.Tensor, out: Optional[torch.Tensor] = None):
    """A[i, j] = sum_d (x[i, d] - x[j, d])^2 of fp32 [n, D] rows (mmg_tsne_sqdist): the difference form in fp64, rounded
    once to fp32, exactly symmetric with a zero diagonal -> fp32 [n, n] (out: the buffer to fill, rows may be padded)."""
    px, n, D, ld = _rows_matrix(x, "x")
    if out is None:
        out = torch.empty(n, n, dtype=torch.float32, device=x.device)
    pa, na, ld_a = _tsne_square(out, "out")
    if na != n:
        raise ValueError(f"tsne_sqdist: out must be [{n}, {n}]")
    _call("mmg_tsne_sqdist", px, n, D, ld, pa, ld_a)                                # takes no workspace: ws = NULL
    return out


def tsne_joint_p(a: torch.Tensor, perplexity: float):
    """The squared distances a [n, n] become the joint probabilities IN PLACE (mmg_tsne_joint_p: sklearn's binary search
    per row, then the symmetrisation) -> (beta fp64 [n], steps int32 [n])."""
    pa, n, ld = _tsne_square(a, "a")
    beta = torch.empty(n, dtype=torch.float64, device=a.device)
    steps = torch.empty(n, dtype=torch.int32, device=a.device)
    _call("mmg_tsne_joint_p", pa, n, ld, float(perplexity), beta, steps, ws=_lib.load().mmg_tsne_joint_p_ws_bytes(n))
    return beta, steps


def tsne_step(a: torch.Tensor, y: torch.Tensor, u: torch.Tensor, g: torch.Tensor, stats: torch.Tensor, exaggeration=1.0,
              momentum=0.8, learning_rate=200.0, min_gain=0.01, want_kl=False, update=True,
              grad_out: Optional[torch.Tensor] = None):
    """One iteration of sklearn's _gradient_descent on _kl_divergence (mmg_tsne_step) over the joint probabilities a
    [n, n]: y, u (the update) and g (the gains) are fp64 [n, 2] and change in place when `update`; stats fp64 [3]
    receives (KL or NaN, sum of the squared gained gradient, Z); grad_out fp64 [n, 2] the gradient before the gains."""
    pa, n, ld = _tsne_square(a, "a")
    for name, t in (("y", y), ("u", u), ("g", g), ("grad_out", grad_out)):
        if t is not None and tuple(t.shape) != (n, 2):
            raise ValueError(f"tsne_step: {name} must be [{n}, 2] (the map has 2 components), got {tuple(t.shape)}")
    if stats.numel() != 3:
        raise ValueError("tsne_step: stats must hold 3 values")
    _call("mmg_tsne_step", pa, n, ld, float(exaggeration), y, u, g, float(momentum), float(learning_rate), float(min_gain),
          int(bool(want_kl)), stats, grad_out, int(bool(update)), ws=_lib.load().mmg_tsne_step_ws_bytes(n))
