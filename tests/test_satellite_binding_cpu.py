"""CPU-side checks of the one binding behind the five satellite libraries (mmgnn/_lib.py: Binding; mmgnn/ops.py: _call):
each header parses, names only symbols its built library defines and keeps the ws / ws_bytes / stream invariant, and
ops._call treats a satellite's prototypes as it treats libmmgnn.so's (no kernel runs here)."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib, ops

STEMS = ["nn", "cluster", "conformal", "boot", "stack"]
# per library: a prototype with a workspace, its arguments (the first a 4-element host tensor handed to a scalar pointer,
# every pointer behind it None) and the header's name of that first parameter
REAL = {"nn": ("mmg_nn_search", (4, 1, 1, None, 4, 0, 1, None, 1, None, 1), "X"),
        "cluster": ("mmg_km_assign", (4, 1, 1, None, 1, None, None, None, None), "X"),
        "conformal": ("mmg_cf_fit", (None, None, None, 8, 4, 1, None, 4, None, 1, 0.1, 0, 0, None, None, None, None), "pred"),
        "boot": ("mmg_boot_sums", (None, None, 0, None, None, 8, 4, 4, 1, 1, 0, None, None), "pred"),
        "stack": ("mmg_stack_scores", (None, None, None, None, 8, 4, 1, None, 4, None, 1, None, None), "raw")}


def module(stem):
    return importlib.import_module(f"mmgnn.{stem}_ops")


@pytest.mark.parametrize("stem", STEMS)
def test_the_header_parses_and_names_what_the_library_defines(stem):
    m = module(stem)
    b = m.BINDING
    assert isinstance(b, _lib.Binding) and b.stem == stem
    assert (m.LIB_PATH, m.HEADER_PATH) == (b.lib_path, b.header_path)
    assert os.path.basename(b.lib_path) == f"libmmgnn_{stem}.so" and os.path.basename(b.header_path) == f"mmgnn_{stem}.h"
    assert (m.DEFINES, m.SIGNATURES, m.PARAMS) == (b.defines, b.signatures, b.params)
    text = re.sub(r"/\*.*?\*/", "", open(b.header_path).read(), flags=re.S)
    assert sorted(re.findall(r"^\s*#\s*define\s+(MMG_\w+)", text, flags=re.M)) == sorted(b.defines) and b.defines
    for name, v in b.defines.items():
        assert type(v) is int and getattr(m, name) == v
    assert b.signatures and sorted(b.signatures) == sorted(b.params)
    assert not set(b.signatures) & set(_lib.SIGNATURES), "the training library's ABI is the one it had"
    assert os.path.exists(b.lib_path), f"{b.lib_path} is not built (make -C multi-modal-gnn_amd/csrc)"
    ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)               # the satellite links against it
    raw = ctypes.CDLL(b.lib_path)
    for sym in b.signatures:
        assert hasattr(raw, sym), sym
    with_ws = [sym for sym, params in b.params.items() if any(p[0] == "ws" for p in params)]
    assert REAL[stem][0] in with_ws
    for sym in with_ws:
        assert sym + "_ws_bytes" in b.signatures and b.signatures[sym + "_ws_bytes"][0] is ctypes.c_size_t, sym
        assert [p[0] for p in b.params[sym]][-3:] == ["ws", "ws_bytes", "stream"], sym
        assert b.params[sym][-3][1:] == ("void", 1) and b.params[sym][-2][1:] == ("size_t", 0), sym
    assert sorted(ops._plans(b)) == sorted(b.signatures) and ops._plans(b) is ops._plans(b)
    assert ops._PLANS is ops._plans(_lib.MAIN) and "mmg_row_degree" in ops._PLANS


@pytest.fixture
def entered(monkeypatch):
    """Stand-ins for every satellite's functions and the stream: what _call would have handed to the library."""
    seen = []

    def recorder(b):
        class Recorder:
            def __getattr__(self, sym):
                assert sym in b.signatures
                return lambda *args: seen.append((sym, args)) or 0
        return Recorder()

    for stem in STEMS:
        b = module(stem).BINDING
        monkeypatch.setattr(b, "load", lambda b=b: recorder(b))
    monkeypatch.setattr(ops, "_stream", lambda: "the stream")
    return seen


@pytest.mark.parametrize("stem", STEMS)
def test_call_marshals_a_satellite_prototype_like_the_main_librarys(stem, entered):
    m = module(stem)
    sym, rest, first = REAL[stem]
    assert m.PARAMS[sym][0][0] == first and len(rest) + 1 == len(m.PARAMS[sym]) - 3
    with pytest.raises(_lib.MmgError, match=rf"^{first}: expected a HIP device tensor, got cpu"):
        m._call(sym, torch.zeros(4), *rest)
    with pytest.raises(_lib.MmgError, match=rf"^{first}: "):          # with a workspace: nothing is taken for it either
        ops._call(sym, torch.zeros(4), *rest, ws=1 << 30, binding=m.BINDING)
    with pytest.raises(_lib.MmgError, match=r"^the first: "):          # names=: the name a refusal uses instead
        m._call(sym, torch.zeros(4), *rest, names={first: "the first"})
    with pytest.raises(TypeError, match=rf"{sym}: takes {len(rest) + 1} arguments"):
        m._call(sym, None, *rest[:-1])                                 # an argument short
    with pytest.raises(_lib.MmgError, match="workspace"):
        m._call(sym, None, *rest, ws=64)                               # a byte count, and no tensor names the device
    assert entered == []                                               # every refusal: before the library is entered
    m._call(sym, None, *rest)
    (got, args), = entered
    assert got == sym and len(args) == len(m.PARAMS[sym]) and args[0] is None and args[1:-3] == rest
    assert args[-3:] == (None, 0, "the stream")                        # no workspace: NULL, 0; the stream is filled in


def test_a_workspace_for_a_prototype_without_one_is_refused(entered):
    from mmgnn import cluster_ops
    assert not any(p[0] == "ws" for p in cluster_ops.PARAMS["mmg_km_label_dist"])
    with pytest.raises(TypeError, match="mmg_km_label_dist: takes no workspace"):
        cluster_ops._call("mmg_km_label_dist", None, 4, 1, 1, None, 1, None, None, ws=64)
    assert entered == []
    cluster_ops._call("mmg_km_label_dist", None, 4, 1, 1, None, 1, None, None)
    assert entered == [("mmg_km_label_dist", (None, 4, 1, 1, None, 1, None, None, "the stream"))]


@pytest.mark.parametrize("stem", STEMS)
def test_a_missing_satellite_header_is_reported_with_its_own_path(stem, monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_HERE", str(tmp_path / "pkg"))
    want = str(tmp_path / "include" / f"mmgnn_{stem}.h")
    with pytest.raises(_lib.MmgError, match=re.escape(want) + " not found"):
        _lib.Binding(stem)


def test_a_missing_satellite_library_is_reported_with_its_path_and_the_build_command(monkeypatch):
    b = _lib.Binding("nn")
    b.lib_path = os.path.join(os.path.dirname(b.lib_path), "libmmgnn_absent.so")
    monkeypatch.setattr(_lib, "load", lambda: None)                    # libmmgnn.so itself is asked for first
    with pytest.raises(_lib.MmgError, match=re.escape(b.lib_path) + r" not found.*make -C .*csrc"):
        b.load()


@pytest.mark.parametrize("stem", STEMS)
def test_a_parse_refusal_names_the_header_it_read(stem, monkeypatch, tmp_path):
    (tmp_path / "include").mkdir()
    (tmp_path / "include" / f"mmgnn_{stem}.h").write_text("int mmg_f(int a, quux_t b);\n")
    monkeypatch.setattr(_lib, "_HERE", str(tmp_path / "pkg"))
    with pytest.raises(_lib.MmgError, match=rf"^mmgnn_{stem}\.h: unknown type 'quux_t'"):
        _lib.Binding(stem)
    with pytest.raises(_lib.MmgError, match=r"^mmgnn\.h: unknown type 'quux_t'"):      # the default: the main header
        _lib.parse_header("int mmg_f(int a, quux_t b);")
