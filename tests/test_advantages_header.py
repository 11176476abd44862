"""include/rware_hip_advantages.h — the part of the C boundary that declares rw_gae, its argument struct and its flags, and that
rware_hip.h pulls in with an #include — against its description in rware_amd._capi (ADVANTAGE_PROTOTYPES, RwGaeArgs, GAE_*), as
tests/test_minibatch_header.py compares rware_hip_minibatch.h with MINIBATCH_PROTOTYPES.  CPU only; nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess

from rware_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
MAIN = strip(open(os.path.join(INCLUDE, "rware_hip.h")).read())
PART = strip(open(os.path.join(INCLUDE, "rware_hip_advantages.h")).read())
NAME = "rw_gae"
C_TYPES = {"float": C.c_float, "int32_t": C.c_int32}
GCC = ["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INCLUDE]


def struct_fields():
    """[(field name, "pointer" or the ctypes scalar)] of rw_gae_args as the part declares them, in order"""
    body = re.search(r"typedef struct rw_gae_args \{(.*?)\} rw_gae_args;", PART, flags=re.S).group(1)
    fields = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        base = re.match(r"(?:const\s+)?([A-Za-z_0-9]+)\s", decl).group(1)
        for item in decl[decl.index(base) + len(base):].split(","):
            item = item.strip()
            fields.append((item.lstrip("* "), "pointer" if item.startswith("*") else C_TYPES[base]))
    return fields


def test_the_main_header_includes_the_part_once_inside_its_extern_c_block():
    inc = '#include "rware_hip_advantages.h"'
    assert MAIN.count(inc) == 1
    at = MAIN.index(inc)
    assert MAIN.index('extern "C" {') < MAIN.index("typedef struct rw_engine rw_engine;") < at < MAIN.rindex("#ifdef __cplusplus")
    assert "#error" in PART and "RWARE_HIP_H" in PART and "RWARE_HIP_ADVANTAGES_H" in PART   # on its own it says what to include instead
    assert "#define RW_ABI_VERSION 4" in MAIN and _capi.RW_ABI_VERSION == 4
    assert NAME not in MAIN                                      # declared in the part alone


def test_the_prototype_and_the_enum_match_the_part():
    found = re.findall(r"\b(int)\s+(rw_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", PART)
    assert [name for _, name, _ in found] == list(_capi.ADVANTAGE_PROTOTYPES) == [NAME]
    restype, argtypes = _capi.ADVANTAGE_PROTOTYPES[NAME]
    assert restype is C.c_int
    assert [a.strip() for a in found[0][2].split(",")] == ["rw_engine *eng", "const rw_gae_args *args"]
    assert argtypes[0] is C.c_void_p and argtypes[1] is C.POINTER(_capi.RwGaeArgs)
    body = re.search(r"enum rw_gae_flags \{(.*?)\};", PART, flags=re.S).group(1)
    flags = {k: int(v) for k, v in re.findall(r"\b(RW_[A-Z_0-9]+)\s*=\s*(-?\d+)", body)}
    assert flags == {"RW_GAE_NEXT_STEP": _capi.GAE_NEXT_STEP, "RW_GAE_TEAM_REWARD": _capi.GAE_TEAM_REWARD}
    assert (_capi.GAE_NEXT_STEP, _capi.GAE_TEAM_REWARD) == (1, 2)


def test_the_ctypes_structure_has_the_c_structs_fields_size_and_offsets(tmp_path):
    fields = struct_fields()
    assert [n for n, _ in fields] == [n for n, _ in _capi.RwGaeArgs._fields_]
    for (name, c_kind), (_, ct) in zip(fields, _capi.RwGaeArgs._fields_):
        assert ("pointer" if ct is C.c_void_p else ct) == c_kind, name
    lines = ["#include <stddef.h>", '#include "rware_hip.h"',
             f'_Static_assert(sizeof(rw_gae_args) == {C.sizeof(_capi.RwGaeArgs)}, "sizeof(rw_gae_args)");']
    for name, _ in _capi.RwGaeArgs._fields_:
        d = getattr(_capi.RwGaeArgs, name)
        lines.append(f'_Static_assert(offsetof(rw_gae_args, {name}) == {d.offset}, "offset of {name}");')
        lines.append(f'_Static_assert(sizeof(((rw_gae_args *)0)->{name}) == {d.size}, "size of {name}");')
    assert len(lines) == 3 + 2 * 18
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run(GCC + [str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    # ... and the check can fail: one offset moved by four bytes
    src.write_text("\n".join(lines).replace(f"gamma) == {_capi.RwGaeArgs.gamma.offset}", f"gamma) == {_capi.RwGaeArgs.gamma.offset + 4}") + "\n")
    assert subprocess.run(GCC + [str(src)], capture_output=True, text=True).returncode != 0


def test_the_five_tables_are_disjoint():
    tables = [set(t) for t in _capi.ALL_PROTOTYPES + _capi.LATER_PROTOTYPES]
    assert len(tables) == 5 and _capi.LATER_PROTOTYPES == (_capi.ADVANTAGE_PROTOTYPES,)
    assert sum(len(t) for t in tables) == len(set().union(*tables))
    assert all(_capi.ADVANTAGE_PROTOTYPES is not t for t in _capi.ALL_PROTOTYPES) and NAME not in _capi.EXPORTS


def test_the_library_exports_it_and_load_declares_it(tmp_path):
    lib = _capi.load()
    fn = lib.rw_gae
    assert fn.restype is C.c_int and list(fn.argtypes) == list(_capi.ADVANTAGE_PROTOTYPES[NAME][1])
    assert fn(None, C.byref(_capi.RwGaeArgs())) == _capi.RW_ERR_INVALID_ARG          # a NULL engine: refused before anything is touched
    assert fn(None, None) == _capi.RW_ERR_INVALID_ARG
    assert _capi.declare(lib, [NAME, "rw_global_records", "rw_sync"]) == []
    # a library with every entry point but this one: declare() names it, load() raises
    older = [n for t in _capi.ALL_PROTOTYPES for n in t]
    src = tmp_path / "older.c"
    src.write_text("".join(f"int {n}(void) {{ return {_capi.RW_ABI_VERSION}; }}\n" for n in older))
    so = tmp_path / "libolder.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    assert _capi.declare(C.CDLL(str(so)), [NAME, "rw_sync"]) == [NAME]
    try:
        _capi.load(str(so))
    except AttributeError as e:
        assert NAME in str(e)
    else:
        raise AssertionError("load() accepted a library without rw_gae")


def test_a_c11_caller_gets_the_declaration_from_the_main_header(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('#include "rware_hip.h"\n'
                   "int f(rw_engine *e, const float *r, const float *v, const uint8_t *t, float *a) {\n"
                   "    rw_gae_args g = {0};\n"
                   "    g.rewards_dev = r; g.values_dev = v; g.last_values_dev = v + 6; g.terminated_dev = t; g.advantages_dev = a;\n"
                   "    g.n_steps = 3; g.n_envs = 2; g.n_agents = 1; g.n_heads = 1; g.gamma = 0.99f; g.lam = 0.95f;\n"
                   "    g.flags = RW_GAE_NEXT_STEP | RW_GAE_TEAM_REWARD;\n"
                   "    return rw_gae(e, &g);\n}\n")
    out = subprocess.run(GCC + [str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    alone = tmp_path / "alone.c"
    alone.write_text('#include <stdint.h>\n#include "rware_hip_advantages.h"\n')
    out = subprocess.run(GCC + [str(alone)], capture_output=True, text=True)
    assert out.returncode != 0 and "include rware_hip.h" in out.stderr
