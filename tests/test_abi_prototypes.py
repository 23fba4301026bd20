"""CPU: the prototype tables of tdmpc2_amd/native.py (native.PROTOTYPES, one per header under include/) against the declarations
themselves.  Every symbol a header declares has an entry and every entry a declaration; the entry lists as many argtypes as the
declaration has parameters ((void) is none), and its restype is the declared return type."""
import ctypes as C
import os
import re

from tdmpc2_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESTYPE = {"void": None, "int": C.c_int, "uint64_t": C.c_uint64, "const char *": C.c_char_p}


def _declarations(header):
    """{name: (return type, parameter count)} of every function the header declares: comments and preprocessor lines go first, the
    parameter list runs to its matching parenthesis and its top-level commas are counted."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for m in re.finditer(r"\b(tdmpc2_[a-z0-9_]+)\s*\(", text):
        depth, commas, end = 1, 0, m.end()
        while depth:
            ch = text[end]
            depth += (ch == "(") - (ch == ")")
            commas += ch == "," and depth == 1
            end += 1
        params = text[m.end():end - 1].strip()
        ret = re.split(r"[;{}]", text[:m.start()])[-1]
        assert m.group(1) not in out and text[end:].lstrip().startswith(";"), m.group(1)
        out[m.group(1)] = (" ".join(ret.replace("*", " * ").split()), 0 if params in ("", "void") else commas + 1)
    return out


def test_every_declaration_matches_its_entry():
    assert sorted(native.PROTOTYPES) == sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    for header, table in native.PROTOTYPES.items():
        declared = _declarations(header)
        assert set(declared) == set(table), (header, sorted(set(declared) ^ set(table)))
        for name, (ret, nparams) in declared.items():
            argtypes, restype = native.signature(table[name])
            assert len(argtypes) == nparams, (name, nparams, len(argtypes))
            assert ret in RESTYPE, (name, ret)
            assert restype is RESTYPE[ret], (name, ret, restype)
