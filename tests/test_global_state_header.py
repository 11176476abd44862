"""include/rware_hip_global_state.h — the part of the C boundary that declares rw_global_record_bytes, rw_global_records and
rw_global_image_gather and that rware_hip.h pulls in with an #include — against its description in rware_amd._capi
(GLOBAL_STATE_PROTOTYPES, GLOBAL_*), as tests/test_minibatch_header.py compares rware_hip_minibatch.h with MINIBATCH_PROTOTYPES.  CPU
only; nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess

from rware_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
MAIN = strip(open(os.path.join(INCLUDE, "rware_hip.h")).read())
PART = strip(open(os.path.join(INCLUDE, "rware_hip_global_state.h")).read())
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t}
NAMES = ["rw_global_record_bytes", "rw_global_records", "rw_global_image_gather"]


def c_class(decl):
    return "pointer" if "*" in decl or "[" in decl else SCALARS[" ".join(w for w in decl.split() if w != "const")]


def ctypes_class(t):
    return "pointer" if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer) else t


def enum_of(name):
    body = re.search(r"enum %s \{(.*?)\};" % name, PART, flags=re.S).group(1)
    return {k: int(v) for k, v in re.findall(r"\b(RW_[A-Z_0-9]+)\s*=\s*(-?\d+)", body)}


def test_the_main_header_includes_the_part_once_inside_its_extern_c_block():
    inc = '#include "rware_hip_global_state.h"'
    assert MAIN.count(inc) == 1
    at = MAIN.index(inc)
    assert MAIN.index('extern "C" {') < MAIN.index("typedef struct rw_engine rw_engine;") < at < MAIN.rindex("#ifdef __cplusplus")
    assert "#error" in PART and "RWARE_HIP_H" in PART          # on its own it says what to include instead
    assert "#define RW_ABI_VERSION 4" in MAIN and _capi.RW_ABI_VERSION == 4


def test_the_prototypes_and_the_three_enums_match_the_part():
    found = re.findall(r"([A-Za-z_0-9 \*]+?)\b(rw_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", PART)
    assert [name for _, name, _ in found] == list(_capi.GLOBAL_STATE_PROTOTYPES) == NAMES
    for ret, name, args in found:
        args = [re.sub(r"\b[A-Za-z_0-9]+\s*$", "", a.strip()) for a in args.split(",")]
        restype, argtypes = _capi.GLOBAL_STATE_PROTOTYPES[name]
        assert ctypes_class(restype) == c_class(ret), name
        assert [ctypes_class(t) for t in argtypes] == [c_class(a) for a in args], name
    assert enum_of("rw_global_elem") == {"RW_GLOBAL_F32": _capi.GLOBAL_F32, "RW_GLOBAL_U8": _capi.GLOBAL_U8, "RW_GLOBAL_F16": _capi.GLOBAL_F16,
                                         "RW_GLOBAL_BF16": _capi.GLOBAL_BF16}
    assert (_capi.GLOBAL_F32, _capi.GLOBAL_U8, _capi.GLOBAL_F16, _capi.GLOBAL_BF16) == (0, 1, 2, 3)   # 0 and 1: rw_global_image's elem
    assert enum_of("rw_global_flags") == {"RW_GLOBAL_INDEX64": _capi.GLOBAL_INDEX64} and _capi.GLOBAL_INDEX64 == 1
    assert enum_of("rw_global_record_flags") == {"RW_GLOBAL_RECORD_NO_MIRROR": _capi.GLOBAL_RECORD_NO_MIRROR,
                                                 "RW_GLOBAL_RECORD_LOADED_NO_MIRROR": _capi.GLOBAL_RECORD_LOADED_NO_MIRROR}
    assert (_capi.GLOBAL_RECORD_NO_MIRROR, _capi.GLOBAL_RECORD_LOADED_NO_MIRROR) == (1, 2)
    assert _capi.GLOBAL_ELEMS == {"float32": 0, "uint8": 1, "float16": 2, "bfloat16": 3}


def test_the_four_tables_are_disjoint():
    tables = [set(_capi.PROTOTYPES), set(_capi.RESTORE_PROTOTYPES), set(_capi.MINIBATCH_PROTOTYPES), set(_capi.GLOBAL_STATE_PROTOTYPES)]
    assert sum(len(t) for t in tables) == len(set().union(*tables))
    assert tuple(_capi.ALL_PROTOTYPES) == (_capi.PROTOTYPES, _capi.RESTORE_PROTOTYPES, _capi.MINIBATCH_PROTOTYPES, _capi.GLOBAL_STATE_PROTOTYPES)
    for name in NAMES:
        assert not re.search(r"\b%s\b" % name, MAIN), name    # declared in the part alone


def test_the_library_exports_them_and_load_declares_them():
    lib = _capi.load()
    for name in NAMES:
        fn = getattr(lib, name)
        restype, argtypes = _capi.GLOBAL_STATE_PROTOTYPES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    inv = _capi.RW_ERR_INVALID_ARG
    assert inv < 0 and lib.rw_global_record_bytes(None) == inv                                   # a NULL engine: refused before anything is touched
    assert lib.rw_global_records(None, None) == inv
    assert lib.rw_global_image_gather(None, None, 0, None, 0, None, 0, None, 0, 0, None) == inv
    assert _capi.declare(lib, NAMES + ["rw_unpack_obs_gather", "rw_snapshot_restore_indexed", "rw_sync"]) == []


def test_a_c11_caller_gets_the_declarations_from_the_main_header(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('#include "rware_hip.h"\n'
                   "int f(rw_engine *e, uint8_t *tape, const int64_t *i, void *o) {\n"
                   "    const int32_t layers[2] = {RW_LAYER_SHELVES, RW_LAYER_AGENT_DIRECTION}, pad[3] = {2, 32, 32};\n"
                   "    const int32_t rb = rw_global_record_bytes(e);\n"
                   "    if (rb < 0 || rw_global_records(e, tape + 3 * (int64_t)rb) != RW_OK) return 1;\n"
                   "    return rw_global_image_gather(e, tape, 7, i, 3, layers, 2, pad, RW_GLOBAL_BF16, RW_GLOBAL_INDEX64, o)\n"
                   "           + (RW_GLOBAL_RECORD_NO_MIRROR | RW_GLOBAL_RECORD_LOADED_NO_MIRROR);\n"
                   "}\n")
    out = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
