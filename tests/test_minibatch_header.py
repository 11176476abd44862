"""include/rware_hip_minibatch.h — the part of the C boundary that declares rw_unpack_obs_gather and that rware_hip.h pulls in with an
#include — against its description in rware_amd._capi (MINIBATCH_PROTOTYPES, UNPACK_*), as tests/test_restore_header.py compares
rware_hip_restore.h with RESTORE_PROTOTYPES.  CPU only; nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess

from rware_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
MAIN = strip(open(os.path.join(INCLUDE, "rware_hip.h")).read())
PART = strip(open(os.path.join(INCLUDE, "rware_hip_minibatch.h")).read())
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t}
NAME = "rw_unpack_obs_gather"


def c_class(decl):
    return "pointer" if "*" in decl or "[" in decl else SCALARS[" ".join(w for w in decl.split() if w != "const")]


def ctypes_class(t):
    return "pointer" if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer) else t


def enum_of(name):
    body = re.search(r"enum %s \{(.*?)\};" % name, PART, flags=re.S).group(1)
    return {k: int(v) for k, v in re.findall(r"\b(RW_[A-Z_0-9]+)\s*=\s*(-?\d+)", body)}


def test_the_main_header_includes_the_part_once_inside_its_extern_c_block():
    inc = '#include "rware_hip_minibatch.h"'
    assert MAIN.count(inc) == 1
    at = MAIN.index(inc)
    assert MAIN.index('extern "C" {') < MAIN.index("typedef struct rw_engine rw_engine;") < at < MAIN.rindex("#ifdef __cplusplus")
    assert "#error" in PART and "RWARE_HIP_H" in PART          # on its own it says what to include instead
    assert "#define RW_ABI_VERSION 4" in MAIN and _capi.RW_ABI_VERSION == 4


def test_the_prototype_and_the_two_enums_match_the_part():
    found = re.findall(r"([A-Za-z_0-9 \*]+?)\b(rw_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", PART)
    assert [name for _, name, _ in found] == list(_capi.MINIBATCH_PROTOTYPES) == [NAME]
    for ret, name, args in found:
        args = [re.sub(r"\b[A-Za-z_0-9]+\s*$", "", a.strip()) for a in args.split(",")]
        restype, argtypes = _capi.MINIBATCH_PROTOTYPES[name]
        assert ctypes_class(restype) == c_class(ret), name
        assert [ctypes_class(t) for t in argtypes] == [c_class(a) for a in args], name
    assert enum_of("rw_unpack_elem") == {"RW_UNPACK_F32": _capi.UNPACK_F32, "RW_UNPACK_F16": _capi.UNPACK_F16, "RW_UNPACK_BF16": _capi.UNPACK_BF16}
    assert (_capi.UNPACK_F32, _capi.UNPACK_F16, _capi.UNPACK_BF16) == (0, 1, 2)
    assert enum_of("rw_unpack_flags") == {"RW_UNPACK_INDEX64": _capi.UNPACK_INDEX64} and _capi.UNPACK_INDEX64 == 1
    assert _capi.UNPACK_ELEMS == {"float32": 0, "float16": 1, "bfloat16": 2}


def test_the_three_tables_are_disjoint():
    tables = [set(_capi.PROTOTYPES), set(_capi.RESTORE_PROTOTYPES), set(_capi.MINIBATCH_PROTOTYPES)]
    assert sum(len(t) for t in tables) == len(set().union(*tables))
    assert NAME not in MAIN                                   # declared in the part alone


def test_the_library_exports_it_and_load_declares_it():
    lib = _capi.load()
    fn = lib.rw_unpack_obs_gather
    assert fn.restype is C.c_int and list(fn.argtypes) == list(_capi.MINIBATCH_PROTOTYPES[NAME][1])
    assert fn(None, None, 0, 1, None, 0, 0, 0, None) == _capi.RW_ERR_INVALID_ARG          # a NULL engine: refused before anything is touched
    assert _capi.declare(lib, [NAME, "rw_snapshot_restore_indexed", "rw_sync"]) == []


def test_a_c11_caller_gets_the_declaration_from_the_main_header(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('#include "rware_hip.h"\nint f(rw_engine *e, const uint32_t *p, const int64_t *i, void *o) '
                   "{ return rw_unpack_obs_gather(e, p, 7, 2, i, 3, RW_UNPACK_BF16, RW_UNPACK_INDEX64, o); }\n")
    out = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
