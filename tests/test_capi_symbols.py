"""CPU-side check: libkrs_hip.so builds for gfx950, loads, and exports every
symbol include/krs.h declares, and the ctypes prototypes of keras_rs_amd._lib are
the header's (no compute call: there is no GPU here)."""

import ctypes as C
import os
import re

import pytest

from keras_rs_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float}


def _ctype(decl: str, ret: bool = False):
    """ctypes type of a C parameter declaration or return type (any pointer: void*, a `const char*` return: char*)."""
    if "*" in decl:
        return C.c_char_p if ret and decl.replace(" ", "") == "constchar*" else C.c_void_p
    return _SCALARS[re.sub(r"\s+\w+$", "", decl.strip()).replace("const ", "").strip()]


def header_prototypes(text: str) -> dict:
    """{name: (restype, [argtypes])} of every krs_* function the header text declares: comments and `#` lines
    stripped, split on `;`, each statement matched as `ret name(params)`."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    protos = {}
    for stmt in text.split(";"):
        stmt = re.split(r"[{}]", stmt)[-1]          # (what follows `extern "C" {` or a struct / enum body)
        m = re.fullmatch(r"\s*([\w\s]+?\**)\s*\b(krs_\w+)\s*\(([^()]*)\)\s*", stmt)
        if m:
            ret, name, params = m.group(1), m.group(2), " ".join(m.group(3).split())
            args = [] if params in ("", "void") else [_ctype(p) for p in params.split(",")]
            assert name not in protos, f"{name} declared twice"
            protos[name] = (_ctype(ret, ret=True), args)
    return protos


def _header():
    return open(os.path.join(ROOT, "include", "krs.h")).read()


def _declared():
    return sorted(header_prototypes(_header()))


def test_header_and_symbol_list_agree():
    # (every `krs_name(` outside a comment is a declaration header_prototypes read)
    called = set(re.findall(r"\b(krs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert _declared() == sorted(called) == sorted(L.SYMBOLS)


def _mismatches(protos: dict, table: dict) -> list:
    bad = [f"{n}: declared, no row" for n in protos if n not in table]
    bad += [f"{n}: row, not declared" for n in table if n not in protos]
    for name in set(protos) & set(table):
        (ret, args), (restype, argtypes) = protos[name], table[name]
        if restype is not ret:
            bad.append(f"{name}: returns {ret.__name__}, row says {restype.__name__}")
        if len(args) != len(argtypes) or any(a is not b for a, b in zip(args, argtypes)):
            bad.append(f"{name}: ({', '.join(a.__name__ for a in args)}) against row "
                       f"({', '.join(b.__name__ for b in argtypes)})")
    return bad


def test_prototype_table_matches_header_entry_by_entry():
    protos = header_prototypes(_header())
    assert _mismatches(protos, L.PROTOTYPES) == []
    # the comparison notices one edited row and one declaration without a row
    edited = dict(L.PROTOTYPES)
    restype, argtypes = edited["krs_gemm"]
    edited["krs_gemm"] = (restype, argtypes[:2] + [C.c_int64] + argtypes[3:])      # a_is_km: int -> int64_t
    assert _mismatches(protos, edited) == [f"krs_gemm: ({', '.join(a.__name__ for a in protos['krs_gemm'][1])}) against "
                                           f"row ({', '.join(b.__name__ for b in edited['krs_gemm'][1])})"]
    extra = header_prototypes(_header().replace("#endif /* KRS_H_ */", "int krs_new_entry(const void* p, float x);\n"))
    assert _mismatches(extra, L.PROTOTYPES) == ["krs_new_entry: declared, no row"]


def test_library_exports_every_declared_symbol():
    from keras_rs_amd.build import build

    build()
    lib = L.lib()
    for name in _declared():
        assert hasattr(lib, name), f"libkrs_hip.so does not export {name}"
    assert lib.krs_version() == 100


def test_struct_layouts_match_header():
    assert L.TABLE_DT.itemsize == 32 and L.FEATURE_DT.itemsize == 24
    import ctypes

    assert ctypes.sizeof(L.GemmEpilogue) == 80


def test_typed_binding_refuses_a_wrong_argument_count_or_kind():
    from keras_rs_amd.build import build

    build()
    fn = L.lib().krs_gemm_workspace_bytes           # host only: sizes a workspace, launches nothing
    assert fn(1, 2, 3, 0) == 0
    with pytest.raises(TypeError):
        fn(1, 2, 3)                                  # a missing argument
    with pytest.raises((TypeError, C.ArgumentError)):
        fn(1, 2, 3.5, 0)                             # a float for int64_t (ctypes: ArgumentError "TypeError: wrong type")
