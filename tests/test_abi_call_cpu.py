"""CPU-side checks of the call layer: the parameter table mmgnn/_lib.py keeps beside SIGNATURES, the ws / ws_bytes / stream
invariant ops._call relies on, and what _call does with host tensors, non-tensors and None (no kernel runs here)."""
import ctypes

import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib, ops

# uint16_t is the one scalar of the header without a torch dtype: mask_r points into int64 storage
NO_DTYPE = {("mmg_rel_mask_build", "mask_r")}


def test_every_prototype_has_its_parameter_table():
    assert sorted(_lib.PARAMS) == sorted(_lib.SIGNATURES) and len(_lib.PARAMS) >= 96
    for sym, params in _lib.PARAMS.items():
        argtypes = _lib.SIGNATURES[sym][1]
        assert len(params) == len(argtypes), sym
        for (name, base, depth), ct in zip(params, argtypes):
            assert name and isinstance(depth, int), (sym, name)
            if depth == 0 and base in _lib._SCALARS:
                assert ct is _lib._SCALARS[base], (sym, name)
    assert _lib.PARAMS["mmg_row_degree"] == [("rowptr", "int32_t", 1), ("n_rows", "int64_t", 0), ("deg", "int32_t", 1),
                                             ("inv_deg", "float", 1), ("stream", "void", 1)]
    assert _lib.PARAMS["mmg_counters_add"][0] == ("counters", "int64_t", 2)


def test_every_scalar_pointer_parameter_has_a_torch_dtype():
    missing = {(sym, name) for sym, params in _lib.PARAMS.items() for name, base, depth in params
               if depth == 1 and base in _lib._SCALARS and base not in _lib.TORCH_DTYPES}
    assert missing == NO_DTYPE
    for base, names in _lib.TORCH_DTYPES.items():
        assert base in _lib._SCALARS and names and all(isinstance(getattr(torch, n), torch.dtype) for n in names)
    want = {"float": torch.float32, "double": torch.float64, "int32_t": torch.int32, "uint32_t": torch.int32,
            "int64_t": torch.int64, "uint64_t": torch.int64, "uint8_t": torch.uint8}
    assert {b: getattr(torch, _lib.TORCH_DTYPES[b][0]) for b in want} == want
    assert _lib.TORCH_DTYPES["uint8_t"] == ("uint8", "bool")


def test_workspace_parameters_are_ws_ws_bytes_stream_in_the_real_header():
    with_ws = [sym for sym, params in _lib.PARAMS.items() if any(p[0] == "ws" for p in params)]
    assert len(with_ws) >= 29
    for sym in with_ws:
        names = [p[0] for p in _lib.PARAMS[sym]]
        i = names.index("ws")
        assert names[i:i + 3] == ["ws", "ws_bytes", "stream"], sym
        assert _lib.PARAMS[sym][i][1:] == ("void", 1) and _lib.PARAMS[sym][i + 1][1:] == ("size_t", 0), sym
    last = [sym for sym in with_ws if _lib.PARAMS[sym][-1][0] != "stream"]
    assert last == ["mmg_linear_wgrad_deferred"] and _lib.PARAMS[last[0]][-1][0] == "job"


@pytest.mark.parametrize("text", [
    "int mmg_f(const float* x,\n          void* ws, void* stream);",                        # ws without ws_bytes
    "int mmg_f(const float* x,\n          void* ws, int n, size_t ws_bytes, void* stream);",  # ws_bytes not directly behind
    "int mmg_f(const float* x,\n          void* ws, size_t ws_bytes);",                     # ws without stream
])
def test_a_header_that_breaks_the_workspace_invariant_is_refused(text):
    with pytest.raises(_lib.MmgError, match="mmg_f"):
        _lib.parse_header(text)
    params = {}
    _lib.parse_header("int mmg_f(const float* x,\n          void* ws, size_t ws_bytes, void* stream);", params)
    assert params == {"mmg_f": [("x", "float", 1), ("ws", "void", 1), ("ws_bytes", "size_t", 0), ("stream", "void", 1)]}


@pytest.fixture
def entered(monkeypatch):
    """Stand-ins for the library's functions and the stream: what _call would have handed to the library."""
    seen = []

    class Recorder:
        def __getattr__(self, sym):
            assert sym in _lib.SIGNATURES
            return lambda *args: seen.append((sym, args)) or 0

    monkeypatch.setattr(_lib, "load", lambda: Recorder())
    monkeypatch.setattr(ops, "_stream", lambda: "the stream")
    return seen


def test_a_host_tensor_is_refused_under_the_headers_name_before_the_library_is_entered(entered):
    rowptr = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(_lib.MmgError, match=r"^rowptr: expected a HIP device tensor, got cpu"):
        ops.row_degree(rowptr)
    with pytest.raises(_lib.MmgError, match=r"^inv_deg: expected a HIP device tensor"):
        ops._call("mmg_row_degree", None, 4, None, torch.zeros(4))
    with pytest.raises(_lib.MmgError, match=r"^b: "):                   # with a workspace: nothing is taken for it either
        ops._call("mmg_order_stats", None, torch.zeros(8), 8, None, 0, None, None, ws=1 << 30)
    with pytest.raises(_lib.MmgError, match=r"^group: "):               # a name the wrapper keeps over the header's
        ops.lab_stats(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.float64), 1, 2)
    assert [sym for sym, _ in entered] == ["mmg_lab_stats_ws_bytes"]    # the size query is host arithmetic, asked directly


def test_non_tensors_pass_through_and_none_is_null(entered):
    rk = (ctypes.c_int64 * 2)(0, 1)
    ptr = ctypes.c_void_p(4096)
    ops._call("mmg_order_stats", ptr, None, 8, rk, 2, None, None)
    (sym, args), = entered
    assert sym == "mmg_order_stats" and len(args) == len(_lib.PARAMS[sym])
    assert args[0] is ptr and args[3] is rk and args[1] is None and args[2:5:2] == (8, 2)
    assert args[-3:] == (None, 0, "the stream")                         # no workspace: NULL, 0; the stream is filled in
    assert ctypes.c_void_p.from_param(None) is None                     # ctypes: None is the NULL pointer
    job = _lib.WgradReduceT()
    ref = ctypes.byref(job)
    ops._call("mmg_linear_wgrad_deferred", None, None, None, None, None, 1, 2, 3, 0, ref)
    assert entered[-1][1][-1] is ref and entered[-1][1][-2] == "the stream"       # the one call whose stream is not last
    with pytest.raises(TypeError, match="mmg_row_degree"):
        ops._call("mmg_row_degree", None, 4, None)                       # an argument short
    with pytest.raises(TypeError, match="mmg_row_degree: takes no workspace"):
        ops._call("mmg_row_degree", None, 4, None, None, ws=64)
    with pytest.raises(_lib.MmgError, match="workspace"):
        ops._call("mmg_order_stats", ptr, None, 8, rk, 2, None, None, ws=64)      # no tensor names the device
