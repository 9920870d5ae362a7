"""CPU-side checks of the binding that mmgnn/_lib.py derives from include/mmgnn.h: the struct layouts and the constants
agree with what a C compiler makes of the same header, and the parser refuses what it does not recognise."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import mmgnn  # noqa: F401
from mmgnn import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the Python names the package and the tests construct the descriptors under
ALIASES = ["RelT", "PrologueT", "HeadT", "HeadGradT", "SmallFwdT", "SmallWgradT", "SmallBnT", "SmallBnBwdT", "BnFinT",
           "NextBnT", "FwdEpiT", "PairSavedT", "WgradReduceT", "BnBwdT", "BnBwdWgradT", "PercentileT", "SumJobT"]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mmgnn.h")).read(), flags=re.S)


def test_every_struct_and_define_of_the_header_is_derived():
    txt = header_text()
    assert len(re.findall(r"\btypedef\s+struct\b", txt)) == len(_lib.STRUCTS) == len(ALIASES)
    assert sorted(s.__name__ for s in _lib.STRUCTS.values()) == sorted(ALIASES)
    for name, s in _lib.STRUCTS.items():
        assert getattr(_lib, s.__name__) is s and issubclass(s, ctypes.Structure), name
    names = re.findall(r"^\s*#\s*define\s+(MMG_\w+)", txt, flags=re.M)
    assert sorted(names) == sorted(_lib.DEFINES) and len(names) == len(set(names))
    for name, v in _lib.DEFINES.items():
        assert type(v) is int and getattr(_lib, name) == v


def test_layouts_and_constants_match_the_c_compiler(tmp_path):
    """sizeof of every struct, offsetof of every field and the value of every MMG_* define, printed by a C program
    generated from the parsed header, against the ctypes layouts and the derived ints."""
    expect, lines = {}, []
    for cname, s in _lib.STRUCTS.items():
        expect[f"sizeof {cname}"] = ctypes.sizeof(s)
        lines.append(f'  printf("sizeof {cname} %lld\\n", (long long)sizeof({cname}));')
        for field, _ in s._fields_:
            expect[f"offsetof {cname} {field}"] = getattr(s, field).offset
            lines.append(f'  printf("offsetof {cname} {field} %lld\\n", (long long)offsetof({cname}, {field}));')
    n_layout = len(expect)
    for name, v in _lib.DEFINES.items():
        expect[f"define {name}"] = v
        lines.append(f'  printf("define {name} %lld\\n", (long long)({name}));')
    assert n_layout >= 166 and len(expect) - n_layout >= 77          # the header as it stood when this was written
    src = tmp_path / "abi_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mmgnn.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc is not None, "no C compiler found (cc, gcc, clang, /opt/rocm/llvm/bin/clang)"
    exe = tmp_path / "abi_layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.splitlines())}
    assert sorted(got) == sorted(expect)
    wrong = {k: (got[k], expect[k]) for k in expect if got[k] != expect[k]}
    assert not wrong, f"(C compiler, derived binding): {wrong}"


@pytest.mark.parametrize("text, word", [
    ("int mmg_f(int a, quux_t b);", "quux_t"),                                  # an unknown type
    ("typedef struct { unsigned x; } mmg_a_t;", "unsigned"),
    ("int mmg_f(int a, int b", "mmg_f"),                                        # an unterminated declaration
    ("typedef struct { int a; int b } mmg_a_t;", "int b"),
    ("int mmg_f(const mmg_a_t* a);\ntypedef struct { int x; } mmg_a_t;", "mmg_a_t"),   # a struct used before it is defined
    ("typedef struct { const mmg_b_t* b; } mmg_a_t;", "mmg_b_t"),
    ("#define MMG_X 1.5", "MMG_X"),                                             # not an int
    ("int mmg_f(int);", "int"),                                                 # nothing is skipped: no unnamed parameter,
    ("static inline int mmg_f(void) { return 0; }", "static"),                  # no function body,
    ("int mmg_f(void);\nint mmg_f(void);", "mmg_f"),                            # no second declaration of a name
])
def test_the_parser_refuses_what_it_does_not_recognise(text, word):
    with pytest.raises(_lib.MmgError, match=re.escape(word)):
        _lib.parse_header(text)


def test_the_parser_reads_the_c_subset_the_header_uses():
    defines, structs, sigs = _lib.parse_header("""
        /* block */ // line
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        extern "C" {
        #define MMG_A (-1)
        #define MMG_B 1u
        typedef struct { int32_t lo, hi; const void* src[4]; const float* g; float* const* pp; } mmg_a_t;
        typedef struct { const mmg_a_t* a; mmg_a_t v; } mmg_b_c_t;
        const char* mmg_s(void);
        size_t mmg_f(const mmg_a_t* a, mmg_a_t v, const float* const* g, void** out,
                     char* names, int n /* why */, uint8_t* m);
        }
        #endif
    """)
    assert defines == {"MMG_A": -1, "MMG_B": 1}
    a, b = structs["mmg_a_t"], structs["mmg_b_c_t"]
    assert (a.__name__, b.__name__) == ("AT", "BCT")
    assert a._fields_ == [("lo", ctypes.c_int32), ("hi", ctypes.c_int32), ("src", ctypes.c_void_p * 4),
                          ("g", ctypes.c_void_p), ("pp", ctypes.POINTER(ctypes.c_void_p))]
    assert b._fields_ == [("a", ctypes.POINTER(a)), ("v", a)]
    assert sigs == {"mmg_s": (ctypes.c_char_p, []),
                    "mmg_f": (ctypes.c_size_t, [ctypes.POINTER(a), a, ctypes.POINTER(ctypes.c_void_p),
                                                ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_void_p])}
    assert sigs["mmg_f"][1][5] is ctypes.c_int


def test_a_missing_header_is_reported_with_its_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "mmgnn.h"))
    with pytest.raises(_lib.MmgError, match=re.escape(str(tmp_path / "include" / "mmgnn.h"))):
        _lib._read_header()
