"""include/rware_hip_restore.h — the part of the C boundary that rware_hip.h pulls in with an #include — against its description in
rware_amd._capi (RESTORE_PROTOTYPES, RESTORE_KEEP_RNG), as tests/test_capi_boundary.py compares the main header with PROTOTYPES; and the
A/B experiments profiles/tools/ab.py carries beside its first seven (MORE_EXPERIMENTS), through the checks tests/test_ab_harness.py makes
of those.  CPU only; nothing here needs a device."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import rware_amd
from rware_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
MAIN = strip(open(os.path.join(INCLUDE, "rware_hip.h")).read())
PART = strip(open(os.path.join(INCLUDE, "rware_hip_restore.h")).read())
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t}


def c_class(decl):
    return "pointer" if "*" in decl or "[" in decl else SCALARS[" ".join(w for w in decl.split() if w != "const")]


def ctypes_class(t):
    return "pointer" if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer) else t


def test_the_main_header_includes_the_part_inside_its_extern_c_block():
    assert MAIN.count('#include "rware_hip_restore.h"') == 1
    at = MAIN.index('#include "rware_hip_restore.h"')
    assert MAIN.index('extern "C" {') < MAIN.index("typedef struct rw_snapshot rw_snapshot;") < at < MAIN.rindex("#ifdef __cplusplus")
    assert "#error" in PART and "RWARE_HIP_H" in PART          # on its own it says what to include instead


def test_prototypes_and_the_flag_match_the_part():
    found = re.findall(r"([A-Za-z_0-9 \*]+?)\b(rw_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", PART)
    assert [name for _, name, _ in found] == list(_capi.RESTORE_PROTOTYPES) == ["rw_snapshot_restore_indexed"]
    assert not set(_capi.RESTORE_PROTOTYPES) & set(_capi.PROTOTYPES)
    for ret, name, args in found:
        args = [re.sub(r"\b[A-Za-z_0-9]+\s*$", "", a.strip()) for a in args.split(",")]
        restype, argtypes = _capi.RESTORE_PROTOTYPES[name]
        assert ctypes_class(restype) == c_class(ret), name
        assert [ctypes_class(t) for t in argtypes] == [c_class(a) for a in args], name
    body = re.search(r"enum rw_restore_flags \{(.*?)\};", PART, flags=re.S).group(1)
    assert dict(re.findall(r"\b(RW_[A-Z_0-9]+)\s*=\s*(-?\d+)", body)) == {"RW_RESTORE_KEEP_RNG": str(_capi.RESTORE_KEEP_RNG)}


def test_the_library_exports_it_and_load_declares_it():
    lib = _capi.load()
    fn = lib.rw_snapshot_restore_indexed
    assert fn.restype is C.c_int and list(fn.argtypes) == list(_capi.RESTORE_PROTOTYPES["rw_snapshot_restore_indexed"][1])
    assert fn(None, None, None, 0) == _capi.RW_ERR_INVALID_ARG          # a NULL engine: refused before anything is touched
    assert _capi.declare(lib, ["rw_snapshot_restore_indexed", "rw_sync"]) == []


def test_a_c_caller_gets_the_declaration_from_the_main_header(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('#include "rware_hip.h"\nint f(rw_engine *e, const rw_snapshot *s, const int32_t *i) '
                   "{ return rw_snapshot_restore_indexed(e, s, i, RW_RESTORE_KEEP_RNG); }\n")
    out = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_further_experiments_resolve_without_a_device():
    spec = importlib.util.spec_from_file_location("ab_harness_more", os.path.join(ROOT, "profiles", "tools", "ab.py"))
    ab = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ab)
    assert set(ab.MORE_EXPERIMENTS) == {"restore_indexed"} and not set(ab.MORE_EXPERIMENTS) & set(ab.EXPERIMENTS)
    for name, exp in ab.MORE_EXPERIMENTS.items():
        assert exp["reps"] >= 1 and exp["configs"] and exp["compare"], name
        for conf in list(exp["configs"].values()) + [s for _, s in exp.get("extras", ())]:
            rware_amd.env_kwargs(conf["env_id"])                                      # registered (KeyError otherwise)
            assert conf.get("mode", "step") in ab.NEEDS and conf.get("fn", "step") in ab.LEG_FUNCTIONS
        for leg in exp["legs"].values():
            assert leg["lib"] in ("parent", "own") and (leg["mode"] is None or leg["mode"] in ab.NEEDS)
            assert _capi.stream_flags(**leg["options"]) >= 0
            assert all(v is True for v in leg["options"].values()), "options are given by keyword, never as numbers"
        for own, parents in exp["compare"]:
            assert exp["legs"][own]["lib"] == "own" and parents and all(exp["legs"][p]["lib"] == "parent" for p in parents), name
    exp = ab.MORE_EXPERIMENTS["restore_indexed"]
    assert exp["configs"] is ab.THREE and exp["legs"] is ab.PARENT_OWN_PARENT       # the per-step legs are `baseline`'s
    assert [(s["fn"], s["envs"]) for _, s in exp["extras"]] == [("restore", 16384), ("restore", 262144), ("restore", 16384)]
