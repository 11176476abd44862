"""rware_amd._capi describes the C boundary once — PROTOTYPES, RwConfig / RwInfo, the RW_* constants, STREAM_FLAGS — and this file
compares every part of that description with include/rware_hip.h: argument lists, struct layouts, flag and status values.  A drift
there is stack garbage at run time, not an error; here it is a failing CPU test."""
import ctypes as C
import re

import pytest

import c_header as ch
import rware_amd
from rware_amd import _capi

HEADER = ch.read("rware_hip.h")


def test_prototypes_match_the_header():
    want = {p.name: (p.ret, p.args) for p in ch.prototypes(HEADER)}
    assert len(want) == 46 and set(_capi.PROTOTYPES) == set(want)
    assert _capi.EXPORTS == tuple(_capi.PROTOTYPES)
    for name, (ret, args) in want.items():
        restype, argtypes = _capi.PROTOTYPES[name]
        assert ch.ctypes_class(restype) == ret, f"{name}: return type"
        assert len(argtypes) == len(args), f"{name}: {len(argtypes)} arguments described, {len(args)} declared"
        for k, (got, exp) in enumerate(zip(argtypes, args)):
            assert ch.ctypes_class(got) == exp, f"{name}: argument {k} is {got}, the header declares {exp}"


@pytest.mark.parametrize("struct, cls, n_decls", [("rw_config", _capi.RwConfig, 24), ("rw_info", _capi.RwInfo, 17)])
def test_structures_match_the_header(struct, cls, n_decls):
    n, want = ch.struct(HEADER, struct)
    assert n == n_decls
    got = []
    for field, t in cls._fields_:
        if issubclass(t, C.Array):
            got.append((field, t._type_, t._length_))
        else:
            got.append((field, ch.ctypes_class(t), None))
    assert got == want


def test_flags_status_and_version_match_the_header():
    flags = ch.enum(HEADER, "rw_stream_flags")
    assert len(flags) == 15
    consts = {n: v for n, v in vars(_capi).items() if n.startswith("RW_") and isinstance(v, int)}
    status = {n: v for n, v in consts.items() if n == "RW_OK" or n.startswith("RW_ERR_")}
    assert status == ch.enum(HEADER, "rw_status")
    assert consts.pop("RW_ABI_VERSION") == int(re.search(r"#define RW_ABI_VERSION (\d+)", HEADER).group(1))
    assert {n: v for n, v in consts.items() if n not in status} == flags      # names and values, both directions
    for option, table in _capi.STREAM_FLAGS.items():
        for value, bits in table.items():
            assert bits == 0 or bits in flags.values(), (option, value, bits)
    used = {bits for table in _capi.STREAM_FLAGS.values() for bits in table.values()} - {0}
    assert used == set(flags.values()), "a flag of the header that no option of STREAM_FLAGS sets"


def test_stream_flags_words():
    sf = _capi.stream_flags
    assert sf() == 0
    for option, bit in (("use_given_stream", 1), ("stats", 128), ("obs_packed", 1024), ("episodes", 2048), ("action_mask", 4096),
                        ("obs_image_u8", 8192), ("time_limit_truncates", 16384)):
        assert sf(**{option: True}) == bit and sf(**{option: 1}) == bit and sf(**{option: False}) == 0 and sf(**{option: None}) == 0
    for option, off, on, on_word in (("jit", 8, 16, "force"), ("pipe", 32, 64, "on"), ("wave_priority", 256, 512, "on")):
        assert sf(**{option: None}) == sf(**{option: "auto"}) == 0
        assert sf(**{option: False}) == sf(**{option: "off"}) == off
        assert sf(**{option: True}) == sf(**{option: on_word}) == on
        assert set(_capi.STREAM_FLAGS[option]) == {None, "auto", False, "off", True, on_word}
    assert (sf(obs_stores=None), sf(obs_stores="auto"), sf(obs_stores="cached"), sf(obs_stores="stream")) == (0, 0, 2, 4)
    assert set(_capi.STREAM_FLAGS["obs_stores"]) == {None, "auto", "cached", "stream"}
    every = dict(use_given_stream=True, stats=True, obs_packed=True, episodes=True, action_mask=True, obs_image_u8=True, time_limit_truncates=True)
    assert sf(obs_stores="stream", jit=True, pipe=True, wave_priority=True, **every) == 32469
    assert sf(obs_stores="cached", jit=False, pipe=False, wave_priority=False) == 298
    for bad in (dict(jit="yes"), dict(pipe="force"), dict(wave_priority="force"), dict(obs_stores=True), dict(obs_stores="nt")):
        with pytest.raises(KeyError):     # (what the dictionary look-ups of Engine.__init__ raised)
            sf(**bad)
    with pytest.raises(TypeError):
        sf(no_such_option=True)


def test_make_config_fills_every_field_by_name():
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    lay = rware_amd.layout_from_params(kw["shelf_columns"], kw["shelf_rows"], kw["column_height"])
    cfg = _capi.make_config(abi_version=3, num_envs=32, layout=lay, n_agents=4, sensor_range=1, request_queue_size=5, max_inactivity_steps=None,
                            max_steps=500, reward_type=2, normalised_coordinates=True, autoreset_mode="same_step", device_id=6,
                            envs_per_workgroup=8, threads_per_workgroup=128, stream=0x1000, observation_type=3, image_layers=(5, 0, 2),
                            image_directional=False, msg_bits=7, action_mask=True, jit="off")
    scalars = {f: getattr(cfg, f) for f, t in cfg._fields_ if f not in ("image_layers", "highways", "goals_xy")}
    assert scalars == dict(
        abi_version=3, num_envs=32, grid_h=lay.grid_size[0], grid_w=lay.grid_size[1], n_agents=4, sensor_range=1, request_queue_size=5,
        max_inactivity_steps=0, max_steps=500, reward_type=2, normalised_coordinates=1, autoreset_mode=2, n_goals=len(lay.goals), device_id=6,
        envs_per_workgroup=8, threads_per_workgroup=128, observation_type=3, image_directional=0, n_image_layers=3, msg_bits=7,
        stream_flags=4096 | 8, stream=0x1000)
    assert list(cfg.image_layers) == [5, 0, 2, 0, 0, 0, 0, 0]
    hw, goals = cfg._arrays      # kept alive on the config
    assert (cfg.highways, cfg.goals_xy) == (hw.ctypes.data, goals.ctypes.data)
    assert hw.dtype == "uint8" and hw.size == cfg.grid_h * cfg.grid_w and goals.dtype == "int32" and goals.size == 2 * cfg.n_goals
    default = _capi.make_config(num_envs=1, layout=lay, n_agents=1, sensor_range=1, request_queue_size=1, max_inactivity_steps=3, max_steps=None, reward_type=0)
    assert (default.abi_version, default.autoreset_mode, default.observation_type, default.image_directional, default.stream_flags, default.stream,
            default.max_inactivity_steps, default.max_steps) == (_capi.RW_ABI_VERSION, 1, 1, 1, 0, None, 3, 0)
    with pytest.raises(KeyError):
        _capi.make_config(num_envs=1, layout=lay, n_agents=1, sensor_range=1, request_queue_size=1, max_inactivity_steps=0, max_steps=0, reward_type=0, jit="maybe")


def test_declare_skips_and_reports_what_a_library_lacks(tmp_path):
    import subprocess
    (tmp_path / "old.c").write_text("int rw_abi_version(void) { return %d; }\n" % _capi.RW_ABI_VERSION)
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(tmp_path / "libold.so"), str(tmp_path / "old.c")])
    old = C.CDLL(str(tmp_path / "libold.so"))
    assert _capi.declare(old) == [n for n in _capi.PROTOTYPES if n != "rw_abi_version"] and old.rw_abi_version.argtypes == []
    with pytest.raises(AttributeError, match="undefined symbol: rw_create"):      # load() is for this tree's library: it has them all
        _capi.load(str(tmp_path / "libold.so"))
    lib = _capi.load()
    assert _capi.declare(C.CDLL(lib._name)) == []
    assert _capi.declare(C.CDLL(None), ["rw_create", "rw_sync"]) == ["rw_create", "rw_sync"]     # (the process itself: no rw_* symbol)
    fresh = C.CDLL(lib._name)
    assert _capi.declare(fresh, ["rw_unpack_obs"]) == [] and fresh.rw_unpack_obs.argtypes == list(_capi.PROTOTYPES["rw_unpack_obs"][1])
