"""The parts of the C boundary — every include/rware_hip_*.h, which rware_hip.h pulls in with an #include — against their rows of
rware_amd._capi.HEADERS, as tests/test_capi_boundary.py compares the main header with its row: entry points, enums, structure layouts,
what the library exports, and the part as a C11 caller sees it.  One parametrized test per check; a part added to HEADERS is checked
without a new file (it needs its entry in PARTICULAR).  CPU only; nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import c_header as ch
from rware_amd import _capi

MAIN = ch.read("rware_hip.h")
PARTS = [h for h in _capi.HEADERS if h != "rware_hip.h"]
INV = _capi.RW_ERR_INVALID_ARG

# What is particular to a part: the typedef behind which the main header includes it, the body of a C11 caller (after `#include
# "rware_hip.h"`) that uses everything it declares, and per entry point the calls with a NULL engine, each refused with RW_ERR_INVALID_ARG
# before anything is touched.
PARTICULAR = {
    "rware_hip_restore.h": dict(
        behind="rw_snapshot",
        caller="int f(rw_engine *e, const rw_snapshot *s, const int32_t *i) { return rw_snapshot_restore_indexed(e, s, i, RW_RESTORE_KEEP_RNG); }\n",
        null_calls={"rw_snapshot_restore_indexed": [(None, None, None, 0)]}),
    "rware_hip_minibatch.h": dict(
        behind="rw_engine",
        caller="int f(rw_engine *e, const uint32_t *p, const int64_t *i, void *o) "
               "{ return rw_unpack_obs_gather(e, p, 7, 2, i, 3, RW_UNPACK_BF16, RW_UNPACK_INDEX64, o); }\n",
        null_calls={"rw_unpack_obs_gather": [(None, None, 0, 1, None, 0, 0, 0, None)]}),
    "rware_hip_global_state.h": dict(
        behind="rw_engine",
        caller="int f(rw_engine *e, uint8_t *tape, const int64_t *i, void *o) {\n"
               "    const int32_t layers[2] = {RW_LAYER_SHELVES, RW_LAYER_AGENT_DIRECTION}, pad[3] = {2, 32, 32};\n"
               "    const int32_t rb = rw_global_record_bytes(e);\n"
               "    if (rb < 0 || rw_global_records(e, tape + 3 * (int64_t)rb) != RW_OK) return 1;\n"
               "    return rw_global_image_gather(e, tape, 7, i, 3, layers, 2, pad, RW_GLOBAL_BF16, RW_GLOBAL_INDEX64, o)\n"
               "           + (RW_GLOBAL_RECORD_NO_MIRROR | RW_GLOBAL_RECORD_LOADED_NO_MIRROR);\n"
               "}\n",
        null_calls={"rw_global_record_bytes": [(None,)], "rw_global_records": [(None, None)],
                    "rw_global_image_gather": [(None, None, 0, None, 0, None, 0, None, 0, 0, None)]}),
    "rware_hip_advantages.h": dict(
        behind="rw_engine",
        caller="int f(rw_engine *e, const float *r, const float *v, const uint8_t *t, float *a) {\n"
               "    rw_gae_args g = {0};\n"
               "    g.rewards_dev = r; g.values_dev = v; g.last_values_dev = v + 6; g.terminated_dev = t; g.advantages_dev = a;\n"
               "    g.n_steps = 3; g.n_envs = 2; g.n_agents = 1; g.n_heads = 1; g.gamma = 0.99f; g.lam = 0.95f;\n"
               "    g.flags = RW_GAE_NEXT_STEP | RW_GAE_TEAM_REWARD;\n"
               "    return rw_gae(e, &g);\n}\n",
        null_calls={"rw_gae": [(None, C.byref(_capi.RwGaeArgs())), (None, None)]}),
}
# the values the binding's constants must have, whatever the headers say (names as the enums of HEADERS spell them) ...
LITERALS = {
    "rw_restore_flags": {"RW_RESTORE_KEEP_RNG": 1},
    "rw_unpack_elem": {"RW_UNPACK_F32": 0, "RW_UNPACK_F16": 1, "RW_UNPACK_BF16": 2}, "rw_unpack_flags": {"RW_UNPACK_INDEX64": 1},
    "rw_global_elem": {"RW_GLOBAL_F32": 0, "RW_GLOBAL_U8": 1, "RW_GLOBAL_F16": 2, "RW_GLOBAL_BF16": 3}, "rw_global_flags": {"RW_GLOBAL_INDEX64": 1},
    "rw_global_record_flags": {"RW_GLOBAL_RECORD_NO_MIRROR": 1, "RW_GLOBAL_RECORD_LOADED_NO_MIRROR": 2},
    "rw_gae_flags": {"RW_GAE_NEXT_STEP": 1, "RW_GAE_TEAM_REWARD": 2},
}
# ... an entry point's arguments as the header writes them and its exact ctypes, where "pointer" alone would not pin them ...
EXACT = {"rw_gae": (["rw_engine *eng", "const rw_gae_args *args"], C.c_int, (C.c_void_p, C.POINTER(_capi.RwGaeArgs)))}
# ... and the number of lines of a structure's layout check: 3 + 2 per field
LAYOUT_LINES = {"rw_gae_args": 3 + 2 * 18}


def test_the_rows_are_disjoint_and_cover_the_include_directory():
    assert set(_capi.HEADERS) == {f for f in os.listdir(ch.INCLUDE) if f.endswith(".h")} and set(PARTICULAR) == set(PARTS)
    tables = [set(h.functions) for h in _capi.HEADERS.values()]
    assert sum(len(t) for t in tables) == len(set().union(*tables))
    assert _capi.HEADERS["rware_hip.h"].functions is _capi.PROTOTYPES and _capi.EXPORTS == tuple(_capi.PROTOTYPES)
    assert _capi.UNPACK_ELEMS == {"float32": 0, "float16": 1, "bfloat16": 2}                     # (the dtype names of the element enums)
    assert _capi.GLOBAL_ELEMS == {"float32": 0, "uint8": 1, "float16": 2, "bfloat16": 3}


@pytest.mark.parametrize("part", PARTS)
def test_the_main_header_includes_the_part_once_inside_its_extern_c_block(part):
    text, inc = ch.read(part), '#include "%s"' % part
    assert MAIN.count(inc) == 1
    typedef = "typedef struct {0} {0};".format(PARTICULAR[part]["behind"])
    assert MAIN.index('extern "C" {') < MAIN.index(typedef) < MAIN.index(inc) < MAIN.rindex("#ifdef __cplusplus")
    assert "#error" in text and "RWARE_HIP_H" in text and part.upper().replace(".", "_") in text   # on its own it says what to include instead
    assert "#define RW_ABI_VERSION 4" in MAIN and _capi.RW_ABI_VERSION == 4
    for name in _capi.HEADERS[part].functions:                                                   # declared in the part alone
        assert not re.search(r"\b%s\b" % name, MAIN) and name not in _capi.PROTOTYPES, name


@pytest.mark.parametrize("part", PARTS)
def test_the_prototypes_and_the_enums_match_the_part(part):
    text, row = ch.read(part), _capi.HEADERS[part]
    found = ch.prototypes(text)
    assert [p.name for p in found] == list(row.functions) == list(PARTICULAR[part]["null_calls"])
    for p in found:
        restype, argtypes = row.functions[p.name]
        assert ch.ctypes_class(restype) == p.ret, p.name
        assert [ch.ctypes_class(t) for t in argtypes] == p.args, p.name
        if p.name in EXACT:
            assert (p.arg_texts, restype, tuple(argtypes)) == EXACT[p.name]
    assert set(row.enums) == set(re.findall(r"\benum (rw_[a-z_0-9]+) \{", text))
    for name, members in row.enums.items():
        assert members == ch.enum(text, name) == LITERALS[name], name               # names and values, both directions


@pytest.mark.parametrize("part", PARTS)
def test_the_ctypes_structures_have_the_c_structs_fields_sizes_and_offsets(part, tmp_path):
    text, row = ch.read(part), _capi.HEADERS[part]
    assert set(row.structs) == set(re.findall(r"typedef struct (rw_[a-z_0-9]+) \{", text))
    for name, cls in row.structs.items():
        _, fields = ch.struct(text, name)
        assert [n for n, _, _ in fields] == [n for n, _ in cls._fields_]
        for (field, c_kind, length), (_, ct) in zip(fields, cls._fields_):
            assert length is None and ch.ctypes_class(ct) == c_kind, field
        lines = ["#include <stddef.h>", '#include "rware_hip.h"', f'_Static_assert(sizeof({name}) == {C.sizeof(cls)}, "sizeof({name})");']
        for field, _ in cls._fields_:
            d = getattr(cls, field)
            lines.append(f'_Static_assert(offsetof({name}, {field}) == {d.offset}, "offset of {field}");')
            lines.append(f'_Static_assert(sizeof((({name} *)0)->{field}) == {d.size}, "size of {field}");')
        assert len(lines) == LAYOUT_LINES[name]
        src = tmp_path / "layout.c"
        src.write_text("\n".join(lines) + "\n")
        out = ch.gcc(src)
        assert out.returncode == 0, out.stderr
        # ... and the check can fail: the last field's offset moved by four bytes
        field = cls._fields_[-1][0]
        moved = f"{field}) == {getattr(cls, field).offset + 4}"
        src.write_text("\n".join(lines).replace(f"{field}) == {getattr(cls, field).offset}", moved) + "\n")
        assert moved in src.read_text() and ch.gcc(src).returncode != 0


@pytest.mark.parametrize("part", PARTS)
def test_the_library_exports_them_and_load_declares_them(part):
    lib, row = _capi.load(), _capi.HEADERS[part]
    for name, (restype, argtypes) in row.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        for args in PARTICULAR[part]["null_calls"][name]:
            assert INV < 0 and fn(*args) == INV, (name, args)             # a NULL engine: refused before anything is touched
    assert _capi.declare(lib, list(row.functions) + ["rw_sync"]) == []


@pytest.mark.parametrize("part", PARTS)
def test_a_library_without_the_part_is_named_by_declare_and_refused_by_load(part, tmp_path):
    names = list(_capi.HEADERS[part].functions)
    others = [n for h, row in _capi.HEADERS.items() if h != part for n in row.functions]
    src = tmp_path / "older.c"
    src.write_text("".join(f"int {n}(void) {{ return {_capi.RW_ABI_VERSION}; }}\n" for n in others))
    so = tmp_path / "libolder.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    assert _capi.declare(C.CDLL(str(so)), names + ["rw_sync"]) == names
    with pytest.raises(AttributeError, match=r"libolder\.so: undefined symbol: %s$" % names[0]):
        _capi.load(str(so))


@pytest.mark.parametrize("part", PARTS)
def test_a_c11_caller_gets_the_declarations_from_the_main_header_alone(part, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('#include "rware_hip.h"\n' + PARTICULAR[part]["caller"])
    out = ch.gcc(src)
    assert out.returncode == 0, out.stderr
    alone = tmp_path / "alone.c"
    alone.write_text('#include <stdint.h>\n#include "%s"\n' % part)
    out = ch.gcc(alone)
    assert out.returncode != 0 and "include rware_hip.h" in out.stderr
