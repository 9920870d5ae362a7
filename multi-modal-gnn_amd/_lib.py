"""ctypes binding of libmmgnn.so (C ABI: include/mmgnn.h) and, through the same Binding, of the satellite libraries
libmmgnn_<stem>.so beside it (include/mmgnn_<stem>.h).

The library is REQUIRED: there is no CPU or eager-PyTorch fallback anywhere in this
package.  If it is missing, importing the ops raises with the build command.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmmgnn.so")          # assigned before the first load(): the library loaded instead
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mmgnn.h")    # as csrc/Makefile finds it


class MmgError(RuntimeError):
    pass


# The one C-type table of the binding: every scalar include/mmgnn.h uses.  `int` is ctypes.c_int itself.
_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int32_t": C.c_int32,
            "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32,
            "uint64_t": C.c_uint64}
_POINTEES = set(_SCALARS) | {"void", "char"}        # T* of these is an untyped address
# C scalar behind a pointer parameter -> names of the torch dtypes a tensor handed to it may have (the first is the one
# a refusal names).  Seeds and bit-plane words are int64 storage; a bool mask is one byte per element.  uint16_t has no
# entry: the one such parameter (mask_r) points into int64 storage and is converted by hand.
TORCH_DTYPES = {"float": ("float32",), "double": ("float64",), "int": ("int32",), "int32_t": ("int32",),
                "uint32_t": ("int32",), "int64_t": ("int64",), "uint64_t": ("int64",), "uint8_t": ("uint8", "bool")}
_PY_NAMES = {"mmg_bnbwd_t": "BnBwdT", "mmg_bnbwd_wgrad_t": "BnBwdWgradT"}     # where CamelCase of the C name is not it
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*$")


def _ctype(base, stars, structs, what, const=False, is_return=False):
    """C type `base` behind `stars` pointer levels -> ctypes type (structs: the structs declared so far)."""
    if base not in _POINTEES and base not in structs:
        raise MmgError(f"unknown type {base!r} in {what!r}")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and base in structs:
        return structs[base]
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    if stars == 1:
        return C.c_char_p if (is_return and const and base == "char") else C.c_void_p
    if stars == 2 and base in _POINTEES:
        return C.POINTER(C.c_void_p)
    raise MmgError(f"unsupported type in {what!r}")


def _declaration(text, structs, is_param=False):
    """`const T* a`, `T lo, hi`, `T* const* p`, `const void* src[4]` -> [(name, ctypes type, C base type, pointer
    depth)]."""
    m = re.match(r"\s*(const\s+)?(\w+)\b\s*(?:const\b\s*)?(.*)$", text, re.S)
    names = m.group(3).split(",") if m else []
    if not names or (is_param and len(names) != 1):
        raise MmgError(f"cannot split the declaration {text.strip()!r}")
    out = []
    for decl in names:
        d = _DECLARATOR.match(decl.strip())
        if not d or (is_param and d.group(3)):
            raise MmgError(f"cannot split the declaration {text.strip()!r}")
        stars = d.group(1).count("*")
        t = _ctype(m.group(2), stars, structs, text.strip(), bool(m.group(1)))
        out.append((d.group(2), t * int(d.group(3)) if d.group(3) else t, m.group(2), stars))
    return out


def parse_header(text, params=None, name="mmgnn.h"):
    """The C subset of include/mmgnn.h -> (defines {name: int}, structs {C name: ctypes.Structure subclass},
    signatures {name: (restype, [argtypes])}).  Whatever it does not recognise raises MmgError with the offending text
    behind `name`, the file name of the header read.
    params (a dict): also filled with name -> [(parameter name, C base type, pointer depth)] of every function.
    A workspace is always the three parameters ws, ws_bytes (directly behind it) and stream: the call layer fills them
    by name, so a prototype with `ws` that breaks this is refused like unknown C."""
    try:
        return _parse(text, params)
    except MmgError as e:
        raise MmgError(f"{name}: {e}") from None


def _parse(text, params):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines, structs, signatures = {}, {}, {}

    def directive(m):
        line = m.group(0).strip()
        d = re.match(r"#\s*define\s+(MMG_\w+)\s+\(?\s*(-?\d+)[uU]?\s*\)?$", line)
        if d:
            defines[d.group(1)] = int(d.group(2))
        elif not re.match(r"#\s*(ifndef\s+\w+|ifdef\s+\w+|endif|include\s*<[\w./]+>|define\s+\w+_H)$", line):
            raise MmgError(f"cannot parse the directive {line!r}")
        return ""

    rest = re.sub(r"^[ \t]*#[^\n]*$", directive, text, flags=re.M).strip()
    depth = 0
    while rest:
        m = re.match(r'extern\s+"C"\s*\{', rest)
        if m or (depth and rest[0] == "}"):
            depth += 1 if m else -1
            rest = rest[m.end() if m else 1:].lstrip()
            continue
        m = re.match(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", rest)
        if m:
            body = m.group(1).split(";")
            if body.pop().strip() or m.group(2) in structs:
                raise MmgError(f"cannot parse the struct {m.group(0)!r}")
            fields = [f[:2] for decl in body for f in _declaration(decl, structs)]
            py = _PY_NAMES.get(m.group(2)) or "".join(w.capitalize() for w in m.group(2).split("_")[1:])
            structs[m.group(2)] = type(py, (C.Structure,), {"_fields_": fields})
        else:
            m = re.match(r"(const\s+)?(\w+)\s*(\**)\s*(\w+)\s*\(([^;{}()]*)\)\s*;", rest)
            if not m or m.group(4) in signatures:
                raise MmgError(f"cannot parse the declaration {rest[:120]!r}")
            what = m.group(0)
            res = _ctype(m.group(2), len(m.group(3)), structs, what, bool(m.group(1)), is_return=True)
            decls = [] if m.group(5).strip() == "void" else m.group(5).split(",")
            decls = [_declaration(p, structs, is_param=True)[0] for p in decls]
            names = [d[0] for d in decls]
            if "ws" in names and (names[names.index("ws") + 1:][:1] != ["ws_bytes"] or "stream" not in names):
                raise MmgError(f"{m.group(4)} takes `ws` without `ws_bytes` directly behind it or without `stream`")
            signatures[m.group(4)] = (res, [d[1] for d in decls])
            if params is not None:
                params[m.group(4)] = [(d[0], d[2], d[3]) for d in decls]
        rest = rest[m.end():].lstrip()
    if depth:
        raise MmgError('unbalanced extern "C" block')
    return defines, structs, signatures


def _read_header(path=None):
    path = path or HEADER_PATH
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise MmgError(f"{path} not found: the binding is derived from the header the library is built from "
                       f"({e})") from None


class Binding:
    """One library and the header it is built from: libmmgnn.so and include/mmgnn.h (stem None), or the satellite
    libmmgnn_<stem>.so and include/mmgnn_<stem>.h beside them.  Making one parses the header -- defines {MMG_* name:
    int}, structs, signatures {symbol: (restype, argtypes)} and params {symbol: [(parameter name, C base type, pointer
    depth)]}: the header is the only description of the ABI's layout -- and loads nothing."""

    def __init__(self, stem=None):
        name = f"mmgnn_{stem}" if stem else "mmgnn"
        self.stem = stem
        self.lib_path = os.path.join(_HERE, f"lib{name}.so")
        self.header_path = os.path.join(os.path.dirname(_HERE), "include", f"{name}.h")    # as csrc/Makefile finds it
        self.params = {}
        self.defines, self.structs, self.signatures = parse_header(_read_header(self.header_path), self.params,
                                                                   f"{name}.h")
        self._lib = None

    def load(self):
        """Load the library (once), a satellite after libmmgnn.so, which it uses.  Raises MmgError loudly when it has
        not been built."""
        if self._lib is not None:
            return self._lib
        if self.stem:
            load()
        if not os.path.exists(self.lib_path):
            raise MmgError(
                f"{self.lib_path} not found: the HIP library is mandatory (no CPU fallback). Build it with "
                f"`make -C {os.path.join(_HERE, 'csrc')}` or `python -c 'import __graft_entry__ as g; g.build()'`.")
        # PyTorch (the package's device-memory plumbing) bundles its own HIP runtime.  It has to be in the process BEFORE the
        # first library is mapped: libmmgnn.so then binds to it; mapped first, the library pulls in /opt/rocm's runtime, PyTorch
        # adds its own later, and the second runtime of a process sees no device ("no ROCm-capable device is detected" from the
        # first library call -- `python __graft_entry__.py smoke`, where build() loaded the library before anything imported torch).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(self.lib_path)
        for name, (res, args) in self.signatures.items():
            fn = getattr(lib, name)     # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        self._lib = lib
        return lib


# libmmgnn.so's binding under the names the package reads it by: every MMG_* define (an int), every struct (under its
# Python name, e.g. mmg_bn_fin_t -> BnFinT), SIGNATURES and PARAMS.
MAIN = Binding()
DEFINES, STRUCTS, SIGNATURES, PARAMS = MAIN.defines, MAIN.structs, MAIN.signatures, MAIN.params
globals().update(DEFINES)
globals().update({s.__name__: s for s in STRUCTS.values()})


def load():
    """Load libmmgnn.so (once) from LIB_PATH as it stands at the first call.  Raises MmgError loudly when it has not been
    built."""
    MAIN.lib_path = LIB_PATH
    return MAIN.load()


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().mmg_last_error()
        raise MmgError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")
