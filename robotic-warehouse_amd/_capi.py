"""ctypes binding of include/rware_hip.h (the in-tree equivalent of the stub in INTEGRATION.md).

There is no CPU fallback: if `csrc/librware_hip.so` has not been built this module raises, and
if no HIP device is visible `rw_create` fails with RW_ERR_NO_DEVICE.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIBRARY = os.path.join(_HERE, "csrc", "librware_hip.so")

RW_ABI_VERSION = 4
RW_OK, RW_ERR_INVALID_ARG, RW_ERR_INVALID_ACTION, RW_ERR_HIP, RW_ERR_UNSUPPORTED, RW_ERR_NO_DEVICE, RW_ERR_INDEX, RW_ERR_SELFTEST = 0, -1, -2, -3, -4, -5, -6, -7

# Every RW_BUF_* kind of include/rware_hip.h, once: name -> (kind id, dtype, shape as a function of the engine's sizes, role).
# Roles: "state" is what reset() / step() evolve and a snapshot holds, "view" a derived view of it (both writable: set_state takes
# them), "io" the launches' inputs and outputs.  Where a kind exists only with a flag (empty otherwise) the comment names it.
_b, _bn, _bn6, _obs = (lambda e: (e.B,)), (lambda e: (e.B, e.N)), (lambda e: (e.B, e.N, 6)), (lambda e: e.obs_shape)
BUFFERS = {
    "obs": (0, np.float32, _obs, "io"),  # not with RW_OBS_PACKED; RW_OBS_IMAGE_U8: uint8 elements (Engine.dtypes overrides this row's dtype)
    "rewards": (1, np.float32, _bn, "io"),
    "terminated": (2, np.uint8, _b, "io"),
    "truncated": (3, np.uint8, _b, "io"),  # read-only
    "grid": (4, np.int32, lambda e: (e.B, 2, e.H, e.W), "view"),
    "agent_x": (5, np.int32, _bn, "view"), "agent_y": (6, np.int32, _bn, "view"), "agent_dir": (7, np.int32, _bn, "view"),
    "agent_carry": (8, np.int32, _bn, "view"), "agent_delivered": (9, np.int32, _bn, "view"),
    "queue": (10, np.int32, lambda e: (e.B, e.Q), "state"),
    "steps": (11, np.int32, _b, "view"), "inactive": (12, np.int32, _b, "view"),
    "rng": (13, np.uint64, lambda e: (6, e.B), "state"),
    "need_reset": (14, np.uint8, _b, "view"),
    "actions": (15, np.int32, lambda e: (e.B, e.N, 1 + e.M) if e.M else (e.B, e.N), "io"),
    "features": (16, np.float32, _bn6, "io"),
    "agent_msg": (17, np.int32, _bn, "state"),
    "final_obs": (18, np.float32, _obs, "io"),  # SAME_STEP autoreset only
    "final_features": (19, np.float32, _bn6, "io"),  # SAME_STEP autoreset with IMAGE_DICT only
    "stat_deliveries": (20, np.int32, _b, "state"), "stat_failed_moves": (21, np.int32, _b, "state"),  # RW_STATS_ON only
    "obs_packed": (22, np.uint32, lambda e: (e.B, e.N, e.PW), "io"),  # RW_OBS_PACKED only; read-only
    "ep_return": (23, np.float32, _bn, "state"), "ep_length": (24, np.int32, _b, "state"),  # RW_EPISODES_ON only (these five)
    "ep_last_return": (25, np.float32, _bn, "state"), "ep_last_length": (26, np.int32, _b, "state"), "ep_count": (27, np.int32, _b, "state"),
    "action_mask": (28, np.uint8, _bn, "io"),  # RW_ACTION_MASK_ON only; read-only
}
BUF = {name: row[0] for name, row in BUFFERS.items()}
BUF_DTYPE = {name: row[1] for name, row in BUFFERS.items()}
WRITABLE_STATE = tuple(name for name, row in BUFFERS.items() if row[3] != "io")  # what WarehouseVecEnv.set_state accepts

RW_STREAM_USE_GIVEN = 1  # rw_stream_flags: `stream` is taken literally, NULL == the device's default stream
RW_OBS_STORES_CACHED, RW_OBS_STORES_STREAM = 2, 4  # rw_stream_flags: keep the observation lines cached / force the non-temporal hint
RW_JIT_OFF, RW_JIT_FORCE = 8, 16  # rw_stream_flags: run-time specialisation (hipRTC) never / always; default: shapes without an exact build, B >= 4096
RW_PIPE_OFF, RW_PIPE_ON = 32, 64  # rw_stream_flags: the chunk-pipelined persistent per-step kernel never / wherever a build exists; default: the engine's measured rule
RW_PRIO_OFF, RW_PRIO_ON = 256, 512  # rw_stream_flags: raised wavefront priority on the chain in front of the first store never / always; default: the engine's measured rule
RW_OBS_PACKED = 1024  # rw_stream_flags: bit-packed FLATTENED observations — uint32 (B, N, PW) in "obs_packed", no float32 "obs" buffer
RW_EPISODES_ON = 2048  # rw_stream_flags: keep per-episode return / length on the device, RW_BUF_EP_RETURN .. _EP_COUNT (off by default)
RW_ACTION_MASK_ON = 4096  # rw_stream_flags: the step kernels write a valid-action byte per agent to RW_BUF_ACTION_MASK (off by default)
RW_OBS_IMAGE_U8 = 8192  # rw_stream_flags: IMAGE / IMAGE_DICT observations as uint8 — "obs" keeps its shape, one byte per element
RW_TIME_LIMIT_TRUNCATES = 16384  # rw_stream_flags: reaching max_steps sets `truncated`, only max_inactivity_steps `terminated` (off by default: the reference's `terminated` = done)
RW_STATS_ON = 128  # rw_stream_flags: keep the per-env event counters RW_BUF_STAT_DELIVERIES / _FAILED_MOVES (off by default)

# rw_config.stream_flags, once: option name (the keyword of Engine / make_config) -> {accepted value: bits}.  A boolean option takes any
# truth value; a tri-state one exactly the spellings listed (anything else is a KeyError); None / "auto" leave the choice to the engine.
_switch = lambda bit: {False: 0, True: bit}
_tri = lambda off, on, on_word: {None: 0, "auto": 0, False: off, "off": off, True: on, on_word: on}
STREAM_FLAGS = {
    "use_given_stream": _switch(RW_STREAM_USE_GIVEN),
    "obs_stores": {None: 0, "auto": 0, "cached": RW_OBS_STORES_CACHED, "stream": RW_OBS_STORES_STREAM},
    "jit": _tri(RW_JIT_OFF, RW_JIT_FORCE, "force"),
    "pipe": _tri(RW_PIPE_OFF, RW_PIPE_ON, "on"),
    "wave_priority": _tri(RW_PRIO_OFF, RW_PRIO_ON, "on"),
    "stats": _switch(RW_STATS_ON), "obs_packed": _switch(RW_OBS_PACKED), "episodes": _switch(RW_EPISODES_ON),
    "action_mask": _switch(RW_ACTION_MASK_ON), "obs_image_u8": _switch(RW_OBS_IMAGE_U8),
    "time_limit_truncates": _switch(RW_TIME_LIMIT_TRUNCATES),
}


def stream_flags(**options) -> int:
    """The rw_config.stream_flags word of these options (the names of STREAM_FLAGS; what is not given is off / the engine's choice)."""
    word = 0
    for name, value in options.items():
        if name not in STREAM_FLAGS:
            raise TypeError(f"stream_flags() got an unexpected option {name!r}")
        table = STREAM_FLAGS[name]
        word |= table[bool(value)] if table.keys() == {False, True} else table[value]
    return word


AUTORESET = {"disabled": 0, None: 0, "next_step": 1, "same_step": 2}


class RwConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "num_envs", "grid_h", "grid_w", "n_agents", "sensor_range",
        "request_queue_size", "max_inactivity_steps", "max_steps", "reward_type",
        "normalised_coordinates", "autoreset_mode", "n_goals", "device_id",
        "envs_per_workgroup", "threads_per_workgroup", "observation_type", "image_directional",
        "n_image_layers")] + [("image_layers", C.c_int32 * 8), ("msg_bits", C.c_int32), ("stream_flags", C.c_int32),
        ("highways", C.c_void_p), ("goals_xy", C.c_void_p), ("stream", C.c_void_p)]


class RwInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "num_envs", "grid_h", "grid_w", "n_agents", "request_queue_size", "n_shelves", "obs_length",
        "envs_per_workgroup", "threads_per_workgroup", "n_workgroups", "lds_bytes", "device_id",
        "compute_units", "specialised", "wave_priority", "build_kind")] + [
        ("algorithmic_bytes_per_env_step", C.c_int64),
        ("device_name", C.c_char * 128), ("arch_name", C.c_char * 64), ("obs_stores_stream", C.c_int32), ("jit", C.c_int32),
        ("engine_bytes_per_env_step", C.c_int64), ("stagger_ticks", C.c_int32), ("pipe_envs_per_workgroup", C.c_int32),
        ("pipe_workgroups", C.c_int32), ("stats", C.c_int32), ("obs_packed", C.c_int32)]


def make_config(*, abi_version=RW_ABI_VERSION, num_envs, layout, n_agents, sensor_range, request_queue_size, max_inactivity_steps, max_steps,
                reward_type, normalised_coordinates=False, autoreset_mode="next_step", device_id=0, envs_per_workgroup=0,
                threads_per_workgroup=0, stream=None, observation_type=1, image_layers=(), image_directional=True, msg_bits=0,
                **flag_options) -> RwConfig:
    """The rw_config of one engine, every field by name; `flag_options` are the options of STREAM_FLAGS.  The returned object keeps the
    `highways` / `goals_xy` arrays it points at alive.  `abi_version`: a caller that drives another build of the library (an A/B
    against a parent commit's) hands in that library's own rw_abi_version()."""
    hw = np.ascontiguousarray(layout.highways, dtype=np.uint8)
    goals = np.ascontiguousarray(np.asarray(layout.goals, dtype=np.int32).reshape(-1))
    cfg = RwConfig(
        abi_version=int(abi_version), num_envs=int(num_envs), grid_h=int(layout.grid_size[0]), grid_w=int(layout.grid_size[1]),
        n_agents=int(n_agents), sensor_range=int(sensor_range), request_queue_size=int(request_queue_size),
        max_inactivity_steps=int(max_inactivity_steps or 0), max_steps=int(max_steps or 0), reward_type=int(reward_type),
        normalised_coordinates=int(bool(normalised_coordinates)), autoreset_mode=AUTORESET[autoreset_mode], n_goals=len(layout.goals),
        device_id=int(device_id), envs_per_workgroup=int(envs_per_workgroup), threads_per_workgroup=int(threads_per_workgroup),
        observation_type=int(observation_type), image_directional=int(bool(image_directional)), n_image_layers=len(image_layers),
        image_layers=(C.c_int32 * 8)(*[int(l) for l in image_layers]), msg_bits=int(msg_bits), stream_flags=stream_flags(**flag_options),
        highways=hw.ctypes.data, goals_xy=goals.ctypes.data, stream=C.c_void_p(stream or 0))
    cfg._arrays = (hw, goals)
    return cfg


# Every entry point of include/rware_hip.h, once: name -> (restype, argtypes), in declaration order.  tests/test_capi_boundary.py compares
# the argument lists, the two structures above and the flag values with the header.
_vp, _i32, _sz, _str, _P = C.c_void_p, C.c_int32, C.c_size_t, C.c_char_p, C.POINTER
PROTOTYPES = {
    "rw_create": (C.c_int, (_P(RwConfig), _P(_vp))),
    "rw_destroy": (C.c_int, (_vp,)),
    "rw_last_error": (_str, (_vp,)),
    "rw_reset": (C.c_int, (_vp, _vp, _vp)),
    "rw_seed_device": (C.c_int, (_vp, _vp, _vp)),
    "rw_reset_device": (C.c_int, (_vp, _vp, _vp)),
    "rw_step": (C.c_int, (_vp, _vp)),
    "rw_step_device": (C.c_int, (_vp, _vp)),
    "rw_step_tape_device": (C.c_int, (_vp, _vp, _i32, _i32, _i32)),
    "rw_step_tape_device_timed": (C.c_int, (_vp, _vp, _i32, _i32, _i32, _i32, _i32)),
    "rw_step_many_device": (C.c_int, (_vp, _vp, _i32, _vp, _vp, _vp)),
    "rw_step_many_device2": (C.c_int, (_vp, _vp, _i32, _vp, _vp, _vp, _vp)),
    "rw_multi_create": (C.c_int, (_P(_vp), _i32, _P(_vp))),
    "rw_multi_step_device": (C.c_int, (_vp, _P(_vp))),
    "rw_multi_destroy": (C.c_int, (_vp,)),
    "rw_device_malloc": (C.c_int, (_vp, _sz, _P(_vp))),
    "rw_device_free": (C.c_int, (_vp, _vp)),
    "rw_copy_to_device": (C.c_int, (_vp, _vp, _vp, _sz)),
    "rw_copy_to_host": (C.c_int, (_vp, _vp, _vp, _sz)),
    "rw_refresh_grid": (C.c_int, (_vp,)),
    "rw_set_stream": (C.c_int, (_vp, _vp)),
    "rw_mark_views_stale": (C.c_int, (_vp,)),
    "rw_refresh_obs": (C.c_int, (_vp,)),
    "rw_unpack_obs": (C.c_int, (_vp, _vp, _vp, C.c_int64)),
    "rw_global_image": (C.c_int, (_vp, _P(_i32), _i32, _P(_i32), _i32, _vp)),
    "rw_sync": (C.c_int, (_vp,)),
    "rw_get_buffer": (C.c_int, (_vp, C.c_int, _P(_vp), _P(_sz))),
    "rw_read": (C.c_int, (_vp, C.c_int, _vp, _sz)),
    "rw_read_outputs": (C.c_int, (_vp, _vp, _vp, _vp, _vp)),
    "rw_read_outputs2": (C.c_int, (_vp, _vp, _vp, _vp, _vp, _vp)),
    "rw_write": (C.c_int, (_vp, C.c_int, _vp, _sz)),
    "rw_recalc_grid": (C.c_int, (_vp, _vp, _i32)),
    "rw_snapshot_create": (C.c_int, (_vp, _P(_vp))),
    "rw_snapshot_save": (C.c_int, (_vp, _vp)),
    "rw_snapshot_restore": (C.c_int, (_vp, _vp)),
    "rw_snapshot_destroy": (C.c_int, (_vp, _vp)),
    "rw_get_info": (C.c_int, (_vp, _P(RwInfo))),
    "rw_jit_log": (_str, (_vp,)),
    "rw_jit_probe": (C.c_int64, (_P(_i32), _str, _str, _sz)),
    "rw_selftest": (C.c_int, (_i32, _str, _sz)),
    "rw_seed_state": (C.c_int, (C.c_uint64, _vp)),
    "rw_event_record": (C.c_int, (_vp, _i32)),
    "rw_event_elapsed_ms": (C.c_int, (_vp, _i32, _i32, _P(C.c_float))),
    "rw_debug_store_floor": (C.c_int, (_vp, _i32, _P(C.c_float))),
    "rw_debug_timeline": (C.c_int, (_vp, _vp, _vp, _P(_i32), _P(_i32))),
    "rw_abi_version": (C.c_int, ()),
}
EXPORTS = tuple(PROTOTYPES)

# What the parts of the boundary (include/rware_hip_*.h, which rware_hip.h includes) add to the constants above: their enums' values ...
RESTORE_KEEP_RNG = 1   # enum rw_restore_flags: RW_RESTORE_KEEP_RNG
UNPACK_F32, UNPACK_F16, UNPACK_BF16 = 0, 1, 2   # enum rw_unpack_elem
UNPACK_INDEX64 = 1                              # enum rw_unpack_flags: RW_UNPACK_INDEX64
UNPACK_ELEMS = {"float32": UNPACK_F32, "float16": UNPACK_F16, "bfloat16": UNPACK_BF16}
GLOBAL_F32, GLOBAL_U8, GLOBAL_F16, GLOBAL_BF16 = 0, 1, 2, 3   # enum rw_global_elem (0 and 1: rw_global_image's `elem`)
GLOBAL_INDEX64 = 1                                            # enum rw_global_flags: RW_GLOBAL_INDEX64
GLOBAL_RECORD_NO_MIRROR, GLOBAL_RECORD_LOADED_NO_MIRROR = 1, 2   # enum rw_global_record_flags: byte H*W of a record
GLOBAL_ELEMS = {"float32": GLOBAL_F32, "uint8": GLOBAL_U8, "float16": GLOBAL_F16, "bfloat16": GLOBAL_BF16}
GAE_NEXT_STEP, GAE_TEAM_REWARD = 1, 2   # enum rw_gae_flags


# ... and their one structure
class RwGaeArgs(C.Structure):
    """rw_gae_args"""
    _fields_ = [(n, C.c_void_p) for n in (
        "rewards_dev", "values_dev", "last_values_dev", "terminated_dev", "truncated_dev", "final_values_dev", "prev_ended_dev",
        "advantages_dev", "returns_dev", "valid_dev")] + [(n, C.c_int32) for n in ("n_steps", "n_envs", "n_agents", "n_heads")] + [
        ("gamma", C.c_float), ("lam", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


# Every header of include/, once: file name -> its entry points (name -> (restype, argtypes), in declaration order), its enums as this
# module mirrors them (C enum name -> {C member: value}, from the constants above: a member is RW_ + the constant's name, or the name
# itself) and its structures (C struct name -> ctypes class).  tests/test_capi_parts.py compares every row but the first with its header,
# as tests/test_capi_boundary.py does the first; declare() and load() look entry points up here, in this order.
Header = collections.namedtuple("Header", "functions enums structs")
_enum = lambda *names: {n if n.startswith("RW_") else "RW_" + n: globals()[n] for n in names}
HEADERS = {
    "rware_hip.h": Header(PROTOTYPES, {
        "rw_status": _enum("RW_OK", "RW_ERR_INVALID_ARG", "RW_ERR_INVALID_ACTION", "RW_ERR_HIP", "RW_ERR_UNSUPPORTED", "RW_ERR_NO_DEVICE",
                           "RW_ERR_INDEX", "RW_ERR_SELFTEST"),
        "rw_stream_flags": _enum("RW_STREAM_USE_GIVEN", "RW_OBS_STORES_CACHED", "RW_OBS_STORES_STREAM", "RW_JIT_OFF", "RW_JIT_FORCE", "RW_PIPE_OFF",
                                 "RW_PIPE_ON", "RW_STATS_ON", "RW_PRIO_OFF", "RW_PRIO_ON", "RW_OBS_PACKED", "RW_EPISODES_ON", "RW_ACTION_MASK_ON",
                                 "RW_OBS_IMAGE_U8", "RW_TIME_LIMIT_TRUNCATES")}, {"rw_config": RwConfig, "rw_info": RwInfo}),
    "rware_hip_restore.h": Header({
        "rw_snapshot_restore_indexed": (C.c_int, (_vp, _vp, _vp, _i32)),
    }, {"rw_restore_flags": _enum("RESTORE_KEEP_RNG")}, {}),
    "rware_hip_minibatch.h": Header({
        "rw_unpack_obs_gather": (C.c_int, (_vp, _vp, C.c_int64, _i32, _vp, C.c_int64, _i32, _i32, _vp)),
    }, {"rw_unpack_elem": _enum("UNPACK_F32", "UNPACK_F16", "UNPACK_BF16"), "rw_unpack_flags": _enum("UNPACK_INDEX64")}, {}),
    "rware_hip_global_state.h": Header({
        "rw_global_record_bytes": (_i32, (_vp,)),
        "rw_global_records": (C.c_int, (_vp, _vp)),
        "rw_global_image_gather": (C.c_int, (_vp, _vp, C.c_int64, _vp, C.c_int64, _P(_i32), _i32, _P(_i32), _i32, _i32, _vp)),
    }, {"rw_global_elem": _enum("GLOBAL_F32", "GLOBAL_U8", "GLOBAL_F16", "GLOBAL_BF16"), "rw_global_flags": _enum("GLOBAL_INDEX64"),
        "rw_global_record_flags": _enum("GLOBAL_RECORD_NO_MIRROR", "GLOBAL_RECORD_LOADED_NO_MIRROR")}, {}),
    "rware_hip_advantages.h": Header({
        "rw_gae": (C.c_int, (_vp, _P(RwGaeArgs))),
    }, {"rw_gae_flags": _enum("GAE_NEXT_STEP", "GAE_TEAM_REWARD")}, {"rw_gae_args": RwGaeArgs}),
}


def declare(lib, names=None):
    """Applies the prototypes of HEADERS (the main header's, or those of `names`) to a CDLL and returns the names that library does not
    export, in table order — a parent commit's library may be older than this description.  No ABI check: that is load()'s."""
    missing = []
    for name in PROTOTYPES if names is None else names:
        restype, argtypes = next(h.functions[name] for h in HEADERS.values() if name in h.functions)
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype, fn.argtypes = restype, list(argtypes)
    return missing


_libs = {}


def _preload_hip_runtime():
    """Keep ONE HIP runtime in the process.  PyTorch-ROCm wheels bundle their own libamdhip64;
    if that copy and /opt/rocm's are both initialised in one process the second one sees no GPUs
    (and device pointers could not be shared zero-copy).  So when torch is installed, its bundled
    runtime is loaded first and librware_hip.so (NEEDED libamdhip64.so.7) binds to it."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            return C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            return None
    return None


def load(path: str | None = None):
    """dlopen the engine library (default: the in-tree gfx950 build) and declare its prototypes."""
    path = os.path.abspath(path or DEFAULT_LIBRARY)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP engine is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C robotic-warehouse_amd/csrc`). There is no CPU fallback.")
    _preload_hip_runtime()
    lib = C.CDLL(path)
    for name in [n for h in HEADERS.values() for n in declare(lib, h.functions)]:  # (this tree's own library has every entry point: what ctypes itself says of a missing one)
        raise AttributeError(f"{path}: undefined symbol: {name}")
    if lib.rw_abi_version() != RW_ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {lib.rw_abi_version()} != {RW_ABI_VERSION}")
    _libs[path] = lib
    return lib


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rware engine error {code}: {msg}")
        self.code = code


class DeviceArray:
    """Borrowed view of an engine buffer; exposes __cuda_array_interface__ so that
    `torch.as_tensor(view, device='cuda')` wraps it without a copy (HIP memory on ROCm torch)."""

    def __init__(self, ptr, shape, dtype, owner):
        self.ptr, self.shape, self.dtype, self._owner = int(ptr), tuple(shape), np.dtype(dtype), owner

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 2, "strides": None}


def selftest(device_id: int = 0, library=None):
    """rw_selftest: the on-device check of the toolchain facts the kernels rely on; returns (ok, message)."""
    lib = load(library)
    log = C.create_string_buffer(1024)
    rc = lib.rw_selftest(int(device_id), log, len(log))
    return rc == RW_OK, log.value.decode()


class Engine:
    """One rw_engine: `num_envs` warehouses on one HIP device."""

    def __init__(self, *, num_envs, layout, n_agents, sensor_range, request_queue_size,
                 max_inactivity_steps, max_steps, reward_type, normalised_coordinates=False,
                 autoreset_mode="next_step", device_id=0, envs_per_workgroup=0,
                 threads_per_workgroup=0, stream=None, library=None, observation_type=1,
                 image_layers=(), image_directional=True, msg_bits=0, use_given_stream=False, obs_stores=None, jit=None, pipe=None, stats=False, wave_priority=None, obs_packed=False, episodes=False, action_mask=False, obs_image_u8=False, time_limit_truncates=False):
        self.lib = load(library)
        self._h = C.c_void_p()
        self._arena, self.arena_allocations = {}, 0  # rollout_host's device tapes (grow-only; freed in close())
        self._index_buf = None  # restore_indexed's device copy of a host index array (upload_index; freed in close())
        cfg = make_config(
            num_envs=num_envs, layout=layout, n_agents=n_agents, sensor_range=sensor_range, request_queue_size=request_queue_size,
            max_inactivity_steps=max_inactivity_steps, max_steps=max_steps, reward_type=reward_type,
            normalised_coordinates=normalised_coordinates, autoreset_mode=autoreset_mode, device_id=device_id,
            envs_per_workgroup=envs_per_workgroup, threads_per_workgroup=threads_per_workgroup, stream=stream,
            observation_type=observation_type, image_layers=image_layers, image_directional=image_directional, msg_bits=msg_bits,
            use_given_stream=use_given_stream, obs_stores=obs_stores, jit=jit, pipe=pipe, stats=stats, wave_priority=wave_priority,
            obs_packed=obs_packed, episodes=episodes, action_mask=action_mask, obs_image_u8=obs_image_u8,
            time_limit_truncates=time_limit_truncates)
        rc = self.lib.rw_create(C.byref(cfg), C.byref(self._h))
        if rc != RW_OK:
            raise EngineError(rc, (self.lib.rw_last_error(None) or b"").decode())
        self.info = RwInfo()
        self._check(self.lib.rw_get_info(self._h, C.byref(self.info)))
        i = self.info
        self.B, self.N, self.Q, self.L, self.S = i.num_envs, i.n_agents, i.request_queue_size, i.obs_length, i.n_shelves
        self.H, self.W = i.grid_h, i.grid_w
        self.M = int(msg_bits)
        win = 2 * int(sensor_range) + 1
        self.obs_shape = (self.B, self.N, self.L) if int(observation_type) == 1 else (self.B, self.N, self.L // (win * win), win, win)
        self.PW = 1 + (self.L + 31) // 32 if int(observation_type) == 1 else 0  # words of a packed row (FLATTENED)
        self.shapes = {name: row[2](self) for name, row in BUFFERS.items()}
        self.stats = bool(i.stats & 1)      # rw_info.stats is a bit set: bit 0 RW_STATS_ON, bit 1 RW_EPISODES_ON
        self.episodes = bool(i.stats & 2)
        self.action_mask = bool(i.stats & 4)  # bit 2 RW_ACTION_MASK_ON
        self.time_limit_truncates = bool(i.stats & 8)  # bit 3 RW_TIME_LIMIT_TRUNCATES: "truncated" is live
        # obs_packed=True (RW_OBS_PACKED): the launches write uint32 rows of PW words to "obs_packed"; "obs" does not exist
        self.packed = i.obs_packed == 1
        # obs_image_u8=True (RW_OBS_IMAGE_U8, rw_info.obs_packed == 2): "obs" holds uint8 elements — this engine's dtype of that row
        self.image_u8 = i.obs_packed == 2
        self.dtypes = dict(BUF_DTYPE, obs=np.uint8) if self.image_u8 else BUF_DTYPE
        self.obs_name = "obs_packed" if self.packed else "obs"  # the observation buffer the launches write

    def _check(self, rc):
        if rc != RW_OK:
            msg = (self.lib.rw_last_error(self._h) or b"").decode()
            if rc == RW_ERR_INVALID_ACTION:
                raise ValueError(msg or "invalid action")
            if rc == RW_ERR_INDEX:  # the reference's IndexError in _make_img_obs (rware/warehouse.py:552,558)
                raise IndexError(msg or "image layer index out of bounds")
            raise EngineError(rc, msg)

    def close(self):
        if self._h:
            for p, _ in self._arena.values():
                self.lib.rw_device_free(self._h, p)
            self._arena = {}
            if self._index_buf is not None:
                self.lib.rw_device_free(self._h, self._index_buf)
                self._index_buf = None
            self.lib.rw_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # hot path -----------------------------------------------------------------------------
    def reset(self, seeds=None, mask=None):
        s = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(self.B))
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(self.B))
        self._check(self.lib.rw_reset(self._h, None if s is None else s.ctypes.data, None if m is None else m.ctypes.data))

    def reset_device(self, seeds_ptr=0, mask_ptr=0):
        """rw_reset_device: reset() from DEVICE arrays — uint64 [B] seeds (0: the envs' own streams continue), uint8 [B] mask (0: all);
        enqueue only (no synchronisation, no host read: legal inside a stream capture).  The arrays must outlive the enqueued work."""
        self._check(self.lib.rw_reset_device(self._h, C.c_void_p(int(seeds_ptr or 0)), C.c_void_p(int(mask_ptr or 0))))

    def seed_device(self, seeds_ptr, mask_ptr=0):
        """rw_seed_device: the envs with a non-zero mask byte (0: all) get the PCG64 state of SeedSequence(seeds[e]); enqueue only."""
        self._check(self.lib.rw_seed_device(self._h, C.c_void_p(int(seeds_ptr or 0)), C.c_void_p(int(mask_ptr or 0))))

    def step_host(self, actions_i32):
        a = np.ascontiguousarray(actions_i32, dtype=np.int32)
        assert a.size == self.B * self.N * (1 + self.M)
        self._check(self.lib.rw_step(self._h, a.ctypes.data))

    def step_device(self, dev_ptr):
        self._check(self.lib.rw_step_device(self._h, C.c_void_p(int(dev_ptr))))

    def step_tape_device(self, tape_ptr, tape_steps, first, n_steps):
        """n_steps per-step launches (rw_step_device each) from a device action tape, issued by one native loop."""
        self._check(self.lib.rw_step_tape_device(self._h, C.c_void_p(int(tape_ptr)), int(tape_steps), int(first), int(n_steps)))

    def step_tape_device_timed(self, tape_ptr, tape_steps, first, n_steps, start_slot, stop_slot):
        """step_tape_device with the timing events attached to the first / last launch (no marker packets)."""
        self._check(self.lib.rw_step_tape_device_timed(self._h, C.c_void_p(int(tape_ptr)), int(tape_steps), int(first),
                                                       int(n_steps), int(start_slot), int(stop_slot)))

    def step_many_device(self, dev_ptr, n_steps, obs_tape=0, reward_tape=0, terminated_tape=0, truncated_tape=0):
        """`truncated_tape`: uint8 [T][B] on the device — every step's flag with time_limit_truncates, zeros without (rw_step_many_device2)."""
        self._check(self.lib.rw_step_many_device2(self._h, C.c_void_p(int(dev_ptr)), int(n_steps),
                                                  C.c_void_p(int(obs_tape)), C.c_void_p(int(reward_tape)),
                                                  C.c_void_p(int(terminated_tape)), C.c_void_p(int(truncated_tape))))

    def rollout_host(self, actions, want_obs=True):
        """`T` fused steps (one launch) from a host action tape (T, B, N); returns host tapes
        (obs (T,B,N,L) or None, rewards (T,B,N), terminated (T,B)) — and truncated (T,B) as a fourth with time_limit_truncates."""
        a = np.ascontiguousarray(actions, dtype=np.int32).reshape(-1, self.B, self.N * (1 + self.M))
        T = a.shape[0]
        obs = np.empty((T,) + self.shapes[self.obs_name], self.dtypes[self.obs_name]) if want_obs else None  # (packed: uint32 (T,B,N,PW))
        rew = np.empty((T, self.B, self.N), np.float32)
        term = np.empty((T, self.B), np.uint8)
        # device tapes from the engine's arena: grow-only buffers kept for the engine's lifetime, so a training loop that
        # calls rollout() with the same T does no device allocation after the first call
        d_a = self._arena_buf("actions", a.nbytes)
        self._check(self.lib.rw_copy_to_device(self._h, d_a, a.ctypes.data, a.nbytes))
        d_o = self._arena_buf("obs", obs.nbytes) if want_obs else C.c_void_p(0)
        d_r, d_t = self._arena_buf("rewards", rew.nbytes), self._arena_buf("terminated", term.nbytes)
        trunc = np.empty((T, self.B), np.uint8) if self.time_limit_truncates else None
        d_u = self._arena_buf("truncated", trunc.nbytes) if trunc is not None else C.c_void_p(0)
        self._check(self.lib.rw_step_many_device2(self._h, d_a, T, d_o, d_r, d_t, d_u))
        if want_obs:
            self._check(self.lib.rw_copy_to_host(self._h, obs.ctypes.data, d_o, obs.nbytes))
        self._check(self.lib.rw_copy_to_host(self._h, rew.ctypes.data, d_r, rew.nbytes))
        self._check(self.lib.rw_copy_to_host(self._h, term.ctypes.data, d_t, term.nbytes))
        if trunc is not None:
            self._check(self.lib.rw_copy_to_host(self._h, trunc.ctypes.data, d_u, trunc.nbytes))
            return obs, rew, term, trunc
        return obs, rew, term

    def _arena_buf(self, name, nbytes):
        ent = self._arena.get(name)
        if ent is None or ent[1] < nbytes:
            if ent is not None:
                self._check(self.lib.rw_device_free(self._h, ent[0]))
                del self._arena[name]
            p = C.c_void_p()
            self._check(self.lib.rw_device_malloc(self._h, nbytes, C.byref(p)))
            ent = self._arena[name] = (p, nbytes)
            self.arena_allocations += 1
        return ent[0]

    def scratch(self, name, nbytes):
        """A device array of at least `nbytes` from the engine's arena (grow-only, kept until release_arena() / close()); a c_void_p."""
        return self._arena_buf(name, nbytes)

    def read_scratch(self, name, host_array):
        """Copies the front of arena buffer `name` into the contiguous `host_array` (waits for the engine's stream)."""
        self._check(self.lib.rw_copy_to_host(self._h, host_array.ctypes.data, self._arena[name][0], host_array.nbytes))

    def create_snapshot(self):
        """An empty snapshot of this engine's size (rw_snapshot_create): a handle for snapshot(into=...)."""
        h = C.c_void_p()
        self._check(self.lib.rw_snapshot_create(self._h, C.byref(h)))
        return h

    def snapshot(self, into=None):
        """Device-resident copy of the whole env state (see rw_snapshot_*); returns an opaque handle."""
        h = self.create_snapshot() if into is None else into
        self._check(self.lib.rw_snapshot_save(self._h, h))
        return h

    def restore(self, handle):
        self._check(self.lib.rw_snapshot_restore(self._h, handle))

    def restore_indexed(self, handle, index_ptr, keep_rng=False):
        """rw_snapshot_restore_indexed: env e takes the state snapshot `handle` holds for env index[e] (-1: keeps its own) — `index_ptr`
        a DEVICE int32 [B] array; `keep_rng`: RW_RESTORE_KEEP_RNG, every env's RNG stream stays as it is.  Enqueue only (no
        synchronisation, no host read: legal inside a stream capture); an index outside -1 .. B-1 shows at the next sync()."""
        self._check(self.lib.rw_snapshot_restore_indexed(self._h, handle, C.c_void_p(int(index_ptr or 0)), RESTORE_KEEP_RNG if keep_rng else 0))

    def upload_index(self, index):
        """A host int32 (B,) index array copied into the device buffer this engine keeps for it (allocated once) -> its device pointer."""
        a = np.ascontiguousarray(index, dtype=np.int32).reshape(self.B)
        if self._index_buf is None:
            p = C.c_void_p()
            self._check(self.lib.rw_device_malloc(self._h, a.nbytes, C.byref(p)))
            self._index_buf = p
        self._check(self.lib.rw_copy_to_device(self._h, self._index_buf, a.ctypes.data, a.nbytes))
        return self._index_buf.value

    def free_snapshot(self, handle):
        self._check(self.lib.rw_snapshot_destroy(self._h, handle))

    def refresh_obs(self):
        self._check(self.lib.rw_refresh_obs(self._h))

    def refresh_grid(self):
        """Brings the exported int32 grid (a derived view) up to date with the steps enqueued so far."""
        self._check(self.lib.rw_refresh_grid(self._h))

    def jit_log(self) -> str:
        return (self.lib.rw_jit_log(self._h) or b"").decode()

    def set_stream(self, stream_handle):
        """Later launches go to `stream_handle` (a hipStream_t as int; 0 = the default stream)."""
        self._check(self.lib.rw_set_stream(self._h, C.c_void_p(int(stream_handle or 0))))

    def mark_views_stale(self):
        """Steps ran that the host side did not see (a replayed HIP graph): the derived views are rebuilt when next asked for."""
        self._check(self.lib.rw_mark_views_stale(self._h))

    def release_arena(self):
        """Frees the device tapes rollout_host() keeps between calls (grow-only otherwise, for the engine's lifetime)."""
        for p, _ in self._arena.values():
            self._check(self.lib.rw_device_free(self._h, p))
        self._arena = {}

    def sync(self):
        self._check(self.lib.rw_sync(self._h))

    # buffers ------------------------------------------------------------------------------
    def read(self, name) -> np.ndarray:
        out = np.empty(self.shapes[name], dtype=self.dtypes[name])
        self._check(self.lib.rw_read(self._h, BUF[name], out.ctypes.data, out.nbytes))
        return out

    def read_outputs(self, want_features=False, want_truncated=False):
        """obs, rewards, terminated (uint8), features-or-None as fresh host arrays: one C call, one synchronisation.  `want_truncated`:
        truncated (uint8) as a fifth element, in the same round trip (rw_read_outputs2)."""
        obs = None if self.packed else np.empty(self.shapes["obs"], self.dtypes["obs"])
        rew = np.empty(self.shapes["rewards"], np.float32)
        term = np.empty(self.shapes["terminated"], np.uint8)
        feat = np.empty(self.shapes["features"], np.float32) if want_features else None
        trunc = np.empty(self.shapes["truncated"], np.uint8) if want_truncated else None
        self._check(self.lib.rw_read_outputs2(self._h, None if self.packed else obs.ctypes.data, rew.ctypes.data, term.ctypes.data,
                                              trunc.ctypes.data if want_truncated else None, feat.ctypes.data if want_features else None))
        if self.packed:  # (rw_read_outputs speaks float32: the packed rows are 1 / 18 of them, one more small copy)
            obs = self.read("obs_packed")
        return (obs, rew, term, feat, trunc) if want_truncated else (obs, rew, term, feat)

    def write(self, name, array):
        a = np.ascontiguousarray(array, dtype=self.dtypes[name]).reshape(self.shapes[name])
        self._check(self.lib.rw_write(self._h, BUF[name], a.ctypes.data, a.nbytes))

    def unpack_obs_device(self, packed_ptr, out_ptr, n_rows):
        """rw_unpack_obs: `n_rows` packed rows (device uint32 [n_rows][PW]) -> float32 [n_rows][L] at `out_ptr`, on the engine's stream."""
        self._check(self.lib.rw_unpack_obs(self._h, C.c_void_p(int(packed_ptr)), C.c_void_p(int(out_ptr)), int(n_rows)))

    def unpack_gather(self, packed_ptr, n_groups, rows_per_group, index_ptr, n_index, elem, index64, out_ptr):
        """rw_unpack_obs_gather: output group i (`rows_per_group` rows of L elements at `out_ptr`, `elem` one of UNPACK_F32 / UNPACK_F16 /
        UNPACK_BF16) <- the unpacked rows of source group index[i] of the device array uint32 [n_groups][rows_per_group][PW] at
        `packed_ptr`; `index_ptr` a DEVICE int32 (`index64`: int64) [n_index] array, 0 / None: the identity.  Enqueue only, one launch
        (legal inside a stream capture); an index outside 0 .. n_groups-1 gives a group of zeros and shows at the next sync()."""
        self._check(self.lib.rw_unpack_obs_gather(self._h, C.c_void_p(int(packed_ptr or 0)), int(n_groups), int(rows_per_group),
                                                  C.c_void_p(int(index_ptr or 0)), int(n_index), int(elem), UNPACK_INDEX64 if index64 else 0,
                                                  C.c_void_p(int(out_ptr or 0))))

    def global_image(self, layers, out_ptr, pad_to_shape=None, dtype=np.float32):
        """rw_global_image: Warehouse.get_global_image of every env, built on the device from the engine's current state into the DEVICE array
        at `out_ptr` — [B][C'][H'][W'] float32 or uint8 (`dtype`), (C', H', W') = `pad_to_shape` or (len(layers), H, W).  Enqueue only (no
        synchronisation, no copy: legal inside a stream capture); an agent the reference would raise IndexError for shows at the next sync()."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError("a global image is float32 or uint8")
        ls = (C.c_int32 * len(layers))(*[int(l) for l in layers])
        pad = None if pad_to_shape is None else (C.c_int32 * 3)(*[int(v) for v in pad_to_shape])
        self._check(self.lib.rw_global_image(self._h, ls, len(layers), pad, 0 if dt == np.float32 else 1, C.c_void_p(int(out_ptr))))

    @property
    def global_record_bytes(self) -> int:
        """rw_global_record_bytes: RB = (H*W + 1 + 15) & ~15, the bytes of one env's global-state record."""
        return int(self.lib.rw_global_record_bytes(self._h))

    def global_records(self, out_ptr):
        """rw_global_records: one record per env — the code byte per cell that rw_global_image expands, a flags byte, zeros — from the
        engine's current state into the DEVICE array uint8 [B][RB] at `out_ptr` (16-byte aligned).  Enqueue only, one launch; the status
        word is not touched."""
        self._check(self.lib.rw_global_records(self._h, C.c_void_p(int(out_ptr or 0))))

    def global_image_gather(self, records_ptr, n_records, index_ptr, n_index, layers, out_ptr, pad_to_shape=None, elem=GLOBAL_F32, index64=False):
        """rw_global_image_gather: output image i ([C'][H'][W'] elements of `elem`, one of GLOBAL_F32 / GLOBAL_U8 / GLOBAL_F16 / GLOBAL_BF16,
        at `out_ptr`) <- the image of record index[i] of the DEVICE array uint8 [n_records][RB] at `records_ptr`; `index_ptr` a DEVICE int32
        (`index64`: int64) [n_index] array, 0 / None: the identity.  Layers and padding as global_image.  Enqueue only, one launch; an index
        outside 0 .. n_records-1 gives an image of zeros and shows at the next sync(), as does a gathered record whose flags say that a
        requested AGENT_DIRECTION / AGENT_LOAD layer had an agent without a mirrored cell (IndexError)."""
        ls = (C.c_int32 * len(layers))(*[int(l) for l in layers])
        pad = None if pad_to_shape is None else (C.c_int32 * 3)(*[int(v) for v in pad_to_shape])
        self._check(self.lib.rw_global_image_gather(self._h, C.c_void_p(int(records_ptr or 0)), int(n_records), C.c_void_p(int(index_ptr or 0)),
                                                    int(n_index), ls, len(layers), pad, int(elem), GLOBAL_INDEX64 if index64 else 0,
                                                    C.c_void_p(int(out_ptr or 0))))

    def gae(self, rewards_ptr, values_ptr, last_values_ptr, terminated_ptr, advantages_ptr, n_steps, n_envs, n_agents, n_heads, *,
            truncated_ptr=0, final_values_ptr=0, prev_ended_ptr=0, returns_ptr=0, valid_ptr=0, gamma=0.99, lam=0.95, next_step=True,
            team_reward=False):
        """rw_gae: GAE(lambda) advantages (and returns, and the valid mask) of the DEVICE tapes rewards float32 [T][B][N], values float32
        [T][B][K], last_values [B][K], terminated / truncated uint8 [T][B], in the operation order include/rware_hip_advantages.h fixes.
        `next_step`: RW_GAE_NEXT_STEP (the tape of a NEXT_STEP autoreset env; `prev_ended_ptr` uint8 [B] chains it to the tape before),
        else a truncated end bootstraps from `final_values_ptr` float32 [T][B][K] (0: from 0).  `team_reward`: RW_GAE_TEAM_REWARD.
        T, B, N, K are the tape's, not the engine's.  Enqueue only, one launch (legal inside a stream capture)."""
        a = RwGaeArgs(int(rewards_ptr or 0) or None, int(values_ptr or 0) or None, int(last_values_ptr or 0) or None,
                      int(terminated_ptr or 0) or None, int(truncated_ptr or 0) or None, int(final_values_ptr or 0) or None,
                      int(prev_ended_ptr or 0) or None, int(advantages_ptr or 0) or None, int(returns_ptr or 0) or None,
                      int(valid_ptr or 0) or None, int(n_steps), int(n_envs), int(n_agents), int(n_heads), float(gamma), float(lam),
                      (GAE_NEXT_STEP if next_step else 0) | (GAE_TEAM_REWARD if team_reward else 0), 0)
        self._check(self.lib.rw_gae(self._h, C.byref(a)))

    def device_array(self, name, dtype=None) -> DeviceArray:
        """`dtype`: present the buffer as another dtype of the same width ("obs_packed" as int32 for torch, whose uint32 has no shift ops)."""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._check(self.lib.rw_get_buffer(self._h, BUF[name], C.byref(ptr), C.byref(nbytes)))
        if name in ("obs", "obs_packed") and not nbytes.value:
            raise RuntimeError('this engine writes packed observations (obs_format="packed"): there is no float32 "obs" buffer — use "obs_packed" and unpack_obs'
                               if name == "obs" else 'this engine writes float32 observations: "obs_packed" exists only with obs_format="packed"')
        return DeviceArray(ptr.value or 0, self.shapes[name], dtype or self.dtypes[name], self)

    def recalc_grid(self, shelf_xy):
        s = np.ascontiguousarray(shelf_xy, dtype=np.int32).reshape(self.B, -1, 2)
        self._check(self.lib.rw_recalc_grid(self._h, s.ctypes.data, s.shape[1]))

    def debug_timeline(self, actions_dev_ptr) -> np.ndarray:
        """uint64 [n_workgroups, n_marks] phase stamps (10 ns ticks) of one step; profiling aid."""
        nwg, nm = C.c_int32(), C.c_int32()
        self._check(self.lib.rw_debug_timeline(self._h, C.c_void_p(int(actions_dev_ptr)), None, C.byref(nwg), C.byref(nm)))
        out = np.zeros((nwg.value, nm.value), dtype=np.uint64)
        self._check(self.lib.rw_debug_timeline(self._h, C.c_void_p(int(actions_dev_ptr)), out.ctypes.data, None, None))
        return out

    def debug_store_floor(self, n_launches=2000) -> float:
        """ms per launch of a kernel that only writes one step's observations (same geometry and store instruction): measurement aid."""
        ms = C.c_float()
        self._check(self.lib.rw_debug_store_floor(self._h, int(n_launches), C.byref(ms)))
        return float(ms.value)

    def event_record(self, slot):
        self._check(self.lib.rw_event_record(self._h, slot))

    def event_elapsed_ms(self, a, b) -> float:
        ms = C.c_float()
        self._check(self.lib.rw_event_elapsed_ms(self._h, a, b, C.byref(ms)))
        return float(ms.value)


class MultiEngine:
    """rw_multi: one C call per step for all the engines of a single-process multi-device env (launcher thread per engine)."""

    def __init__(self, engines):
        self.engines, self.lib = list(engines), engines[0].lib
        n = len(self.engines)
        hs = (C.c_void_p * n)(*[e._h for e in self.engines])
        self._h = C.c_void_p()
        rc = self.lib.rw_multi_create(hs, n, C.byref(self._h))
        if rc != RW_OK:
            raise EngineError(rc, "rw_multi_create failed")
        self._ptrs = (C.c_void_p * n)()

    def step_device(self, dev_ptrs):
        p = self._ptrs
        for k, v in enumerate(dev_ptrs):
            p[k] = v
        rc = self.lib.rw_multi_step_device(self._h, p)
        if rc != RW_OK:
            # (engine 0's message names the engine that failed this round — rw_multi_step_device writes it there on every path;
            #  should it be empty all the same, the first engine that has one)
            msg = (self.lib.rw_last_error(self.engines[0]._h) or b"").decode()
            if not msg:
                msg = next((m for m in ((self.lib.rw_last_error(e._h) or b"").decode() for e in self.engines[1:]) if m), "")
            raise EngineError(rc, msg or "rw_multi_step_device failed")

    def close(self):
        if self._h:
            self.lib.rw_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def seed_state(seed: int, library=None) -> np.ndarray:
    out = np.zeros(6, dtype=np.uint64)
    rc = load(library).rw_seed_state(C.c_uint64(int(seed)), out.ctypes.data)
    assert rc == RW_OK
    return out


def jit_probe(*, sensor_range, H, W, N, Q, S, E, msg_bits=0, obs=0, layers=(), directional=True, nt=1, packed=0, arch="gfx950", library=None):
    """Compile (or find cached) the run-time specialised build of a shape without a device; returns (code bytes or -1, log)."""
    layer_bits = 0
    for k, l in enumerate(layers):
        layer_bits |= int(l) << (4 * k)
    shape = (C.c_int32 * 16)(sensor_range, H, W, N, Q, S, E, 256, msg_bits, 1 if S > 255 else 0, obs, len(layers), layer_bits,
                             (1 if directional else 0) if obs in (1, 3) else -1, nt, int(packed))
    log = C.create_string_buffer(4096)
    n = load(library).rw_jit_probe(shape, arch.encode(), log, 4096)
    return int(n), log.value.decode(errors="replace")
