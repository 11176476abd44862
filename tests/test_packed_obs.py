"""Bit-packed FLATTENED observations (obs_format="packed", RW_OBS_PACKED): the format against the reference's own observations,
the emulated engine against every FLATTENED golden trace, the host layer, the guard on the ahead-of-time kernels' ISA, and — on a
GPU — the generic kernel, the run-time exact-shape packed build and rw_unpack_obs against the goldens and the oracle.

The reference in every comparison is the float32 observation of the golden fixtures (recorded from the unmodified reference) or of
the oracle; every comparison is exact (np.array_equal / torch.equal): unpacking is defined to reproduce RW_BUF_OBS bit for bit."""
import ctypes as C
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

import golden_util as gu
from engine_backend import EngineBackend, build_emu
from oracle_shards import ShardedOracle
from rware_oracle import OracleVecEnv

import rware_amd
from rware_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "profiles", "tools", "isa_stats.py"))
isa_stats = importlib.util.module_from_spec(_spec)      # the tool that recorded tests/golden/isa/*.json: its compile and its figures
_spec.loader.exec_module(isa_stats)
pytestmark = pytest.mark.timeout(1500)


def _flattened_goldens():
    names = []
    for n in gu.fixture_names():
        meta, _ = gu.load_fixture(n)
        if int(meta["kwargs"].get("observation_type", 1) or 1) == 1:  # (FLATTENED: ObservationType value 1; DICT fixtures hold none)
            names.append(n)
    return names


FLAT = _flattened_goldens()


def _pack_args(meta):
    kw = gu.ctor_kwargs(meta)
    lay = rware_amd.layout_from_str(kw["layout"]) if kw.get("layout") else rware_amd.layout_from_params(
        kw.get("shelf_columns", 3), kw.get("shelf_rows", 1), kw.get("column_height", 8))
    return dict(grid_size=lay.grid_size, sensor_range=kw.get("sensor_range", 1), msg_bits=kw.get("msg_bits", 0),
                normalised_coordinates=bool(kw.get("normalised_coordinates", False)))


class PackedBackend(EngineBackend):
    """The replay harness's adapter over an obs_format="packed" env: every observation it hands out is the engine's uint32 rows,
    unpacked — so golden_util.replay compares unpack(packed) with the fixture's float32 observation, exactly, at every step."""

    def __init__(self, *a, **kw):
        super().__init__(*a, obs_format="packed", **kw)
        self.n_obs = 0

    def _obs(self, o):
        o = self._first(o)
        assert o.dtype == np.uint32 and o.shape[-1] == self.env.packed_words, (o.dtype, o.shape)
        L = self.env.obs_length
        assert not (o[..., 1] & 3).any(), "bits 0 and 1 of word 1 (the coordinate slots) must be 0"
        if L % 32:
            assert not (o[..., -1] >> np.uint32(L % 32)).any(), "the bits from L upwards in the last word must be 0"
        self.n_obs += 1
        return self.env.unpack_obs(o)


# ------------------------------------------------------------------------------------------------ CPU: the format
def test_there_are_sixteen_flattened_goldens():
    assert len(FLAT) == 16, FLAT
    assert "small-3ag-normcoord-sr3" in FLAT and any(n.startswith("msg2-") for n in FLAT) and any(n.startswith("msg3-") for n in FLAT)


@pytest.mark.parametrize("name", FLAT)
def test_pack_unpack_round_trips_the_references_observations(name):
    meta, z = gu.load_fixture(name)
    args = _pack_args(meta)
    obs = np.concatenate([z["obs0"][None].astype(np.float32), z["obs"].astype(np.float32)])
    L = obs.shape[-1]
    body = obs[..., 2:]
    assert ((body == 0) | (body == 1)).all()
    p = rware_amd.pack_obs(obs, **args)
    assert p.dtype == np.uint32 and p.shape == obs.shape[:-1] + (1 + (L + 31) // 32,)
    assert p.shape[-1] == rware_amd.packed_words(args["sensor_range"], args["msg_bits"])
    assert not (p[..., 1] & 3).any()
    if L % 32:
        assert not (p[..., -1] >> np.uint32(L % 32)).any()
    back = rware_amd.unpack_obs(p, **args)
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), obs.view(np.uint32))   # bit for bit
    # word 0 holds the cell indices as integers, whatever normalised_coordinates says
    H, W = args["grid_size"]
    assert (p[..., 0] & 0xFFFF).max() < W and (p[..., 0] >> 16).max() < H


def test_unpack_takes_torch_tensors_and_any_leading_dimensions():
    torch = pytest.importorskip("torch")
    meta, z = gu.load_fixture("small-3ag-normcoord-sr3")
    args = _pack_args(meta)
    obs = z["obs"][:7].astype(np.float32)
    p = rware_amd.pack_obs(obs, **args)
    t = torch.from_numpy(p.view(np.int32))          # (the zero-copy views hold the uint32 rows as int32: same bits)
    out = rware_amd.unpack_obs(t, **args)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == t.device
    assert np.array_equal(out.numpy().view(np.uint32), obs.view(np.uint32))
    assert np.array_equal(rware_amd.unpack_obs(t[2, 1], **args).numpy(), obs[2, 1])
    with pytest.raises(ValueError):
        rware_amd.unpack_obs(p[..., :-1], **args)
    with pytest.raises(ValueError):
        rware_amd.pack_obs(obs + 0.5, **args)


# ------------------------------------------------------------------------------------------------ CPU: the emulated engine
@pytest.mark.parametrize("name", FLAT)
def test_emulated_packed_engine_replays_reference_golden(name):
    meta, z = gu.load_fixture(name)
    be = PackedBackend(meta["E"], library=build_emu(), **gu.ctor_kwargs(meta))
    info = be.env.engines[0].info
    assert info.obs_packed == 1 and info.build_kind == 0      # packed rows: never an ahead-of-time specialised build
    # (the first 120 steps of each trace, as tests/test_engine_emulated.py replays them — a workgroup is 256 OS threads here; every
    #  trace runs in FULL, on both kernels, in test_gpu_packed_engine_replays_reference_golden below)
    assert gu.replay(be, meta, z, steps=120) == min(120, meta["T"]) and be.n_obs > 1
    be.env.close()


@pytest.mark.parametrize("geom,B", [((4, 64), 7), ((4, 128), 5), ((16, 256), 40)])   # every batch ends in a partial last workgroup
@pytest.mark.parametrize("mode", ["next_step", "same_step", "disabled"])
def test_emulated_packed_engine_matches_oracle(mode, geom, B):
    kw = dict(rware_amd.env_kwargs("rware-tiny-2ag-v1"), max_steps=12)
    env = rware_amd.WarehouseVecEnv(B, library=build_emu(), autoreset_mode=mode, obs_format="packed", envs_per_workgroup=geom[0],
                                    threads_per_workgroup=geom[1], **kw)
    orc = OracleVecEnv(B, **dict(kw, reward_type=kw["reward_type"].value))
    assert np.array_equal(env.unpack_obs(env.reset(seed=5)[0]), orc.reset(seed=5))
    rng = np.random.default_rng(1)
    n_final = 0
    for t in range(40):
        a = rng.choice(5, size=(B, 2), p=[.1, .5, .15, .15, .1]).astype(np.int32)
        obs, rew, term, _, info = env.step(a)
        o2, r2, d2 = orc.step_autoreset(a, mode)
        assert obs.dtype == np.uint32 and np.array_equal(env.unpack_obs(obs), o2), t
        assert np.array_equal(rew, r2) and np.array_equal(term, d2.astype(bool)), t
        if mode == "same_step" and d2.any():   # the terminal observation stays float32
            m = orc.final_mask
            assert info["final_obs"].dtype == np.float32 and np.array_equal(info["final_obs"][m], orc.final_obs[m]), t
            n_final += int(m.sum())
        if mode == "disabled" and d2.all():
            break
    assert mode != "same_step" or n_final > 0
    env.close()


def test_emulated_unaligned_chunks_take_the_scalar_tail():
    """The 16-byte stores need a chunk that starts on a 16-byte boundary.  rw_create refuses an envs_per_workgroup that is not a
    multiple of 4 (3 is RW_ERR_INVALID_ARG, with or without the flag — unchanged), so through the C-ABI every chunk of the engine's own
    buffer is aligned; a chunk that is NOT arrives with a caller's tape: a rollout into `obs_tape + 1 word` (a slice of a larger buffer)
    sends every word of every chunk through the scalar tail, and has to write the same rows."""
    kw = dict(rware_amd.env_kwargs("rware-tiny-2ag-v1"), max_steps=7)
    with pytest.raises(_capi.EngineError) as ei:
        rware_amd.WarehouseVecEnv(6, library=build_emu(), obs_format="packed", envs_per_workgroup=3, **kw)
    assert ei.value.code == _capi.RW_ERR_INVALID_ARG
    B, T, N = 7, 9, 2
    env = rware_amd.WarehouseVecEnv(B, library=build_emu(), obs_format="packed", envs_per_workgroup=4, threads_per_workgroup=64, **kw)
    ref = rware_amd.WarehouseVecEnv(B, library=build_emu(), envs_per_workgroup=4, threads_per_workgroup=64, **kw)
    env.reset(seed=3); ref.reset(seed=3)
    acts = np.ascontiguousarray(np.random.default_rng(2).integers(0, 5, size=(T, B, N)).astype(np.int32))
    eng = env.engines[0]
    words = T * B * N * eng.PW
    d_a, d_o = C.c_void_p(), C.c_void_p()
    eng._check(eng.lib.rw_device_malloc(eng._h, acts.nbytes, C.byref(d_a)))
    eng._check(eng.lib.rw_device_malloc(eng._h, (words + 4) * 4, C.byref(d_o)))
    eng._check(eng.lib.rw_copy_to_device(eng._h, d_a, acts.ctypes.data, acts.nbytes))
    eng.step_many_device(d_a.value, T, obs_tape=d_o.value + 4)      # 4 bytes off a 16-byte boundary
    tape = np.zeros((T, B, N, eng.PW), np.uint32)
    eng._check(eng.lib.rw_copy_to_host(eng._h, tape.ctypes.data, d_o.value + 4, tape.nbytes))
    for t in range(T):
        assert np.array_equal(env.unpack_obs(tape[t]), ref.step(acts[t])[0]), t
    eng._check(eng.lib.rw_device_free(eng._h, d_a)); eng._check(eng.lib.rw_device_free(eng._h, d_o))
    env.close(); ref.close()


def test_emulated_fused_rollout_refresh_and_snapshot_produce_packed_rows():
    kw = dict(rware_amd.env_kwargs("rware-small-4ag-v1"), max_steps=9)
    B, T = 10, 14
    env = rware_amd.WarehouseVecEnv(B, library=build_emu(), obs_format="packed", **kw)
    ref = rware_amd.WarehouseVecEnv(B, library=build_emu(), **kw)
    env.reset(seed=8); ref.reset(seed=8)
    acts = np.random.default_rng(4).integers(0, 5, size=(T, B, 4)).astype(np.int32)
    tape, rew, term = env.rollout(acts)            # one fused launch; obs_stride counts packed words
    assert tape.dtype == np.uint32 and tape.shape == (T, B, 4, env.packed_words)
    for t in range(T):
        o, r, d, _, _ = ref.step(acts[t])
        assert np.array_equal(env.unpack_obs(tape[t]), o) and np.array_equal(rew[t], r) and np.array_equal(term[t], d), t
    env.engines[0].refresh_obs()    # (a rollout with a tape leaves the engine's own buffer alone — as for float32 rows: OP_OBS recomputes it)
    assert np.array_equal(env.unpack_obs(env.observations()), ref.observations())
    # rw_refresh_obs after set_state: the packed rows follow the injected state
    st = ref.get_state()
    tok = env.snapshot()
    env.reset(seed=99)
    env.set_state(**{k: st[k] for k in st})
    assert np.array_equal(env.unpack_obs(env.observations()), ref.observations())
    # restore recomputes the observation in the engine's format
    env.reset(seed=99)
    assert np.array_equal(env.unpack_obs(env.restore(tok)), ref.observations())
    env.free_snapshot(tok)
    env.close(); ref.close()


def test_emulated_rw_unpack_obs_equals_the_python_unpack():
    for name in ("small-3ag-normcoord-sr3", "msg2-small-4ag", "tiny-2ag"):
        meta, z = gu.load_fixture(name)
        env = rware_amd.WarehouseVecEnv(meta["E"], library=build_emu(), obs_format="packed", **gu.ctor_kwargs(meta))
        eng = env.engines[0]
        env.reset(seed=meta["seed"])
        env.step(z["actions"][0].astype(np.int32))
        packed = env.observations()
        ptr, nb = C.c_void_p(), C.c_size_t()
        eng._check(eng.lib.rw_get_buffer(eng._h, _capi.BUF["obs_packed"], C.byref(ptr), C.byref(nb)))
        assert nb.value == packed.nbytes
        n_rows = eng.B * eng.N
        out = C.c_void_p()
        eng._check(eng.lib.rw_device_malloc(eng._h, n_rows * eng.L * 4 + 16, C.byref(out)))
        for first in (0, 1):      # all rows (16-byte aligned output); from row 1 on (an output that starts off a 16-byte boundary)
            host = np.zeros((n_rows - first, eng.L), np.float32)
            eng.unpack_obs_device(ptr.value + first * eng.PW * 4, out.value + first * eng.L * 4, n_rows - first)
            eng._check(eng.lib.rw_copy_to_host(eng._h, host.ctypes.data, out.value + first * eng.L * 4, host.nbytes))
            want = env.unpack_obs(packed).reshape(n_rows, eng.L)[first:]
            assert np.array_equal(host.view(np.uint32), want.view(np.uint32)), (name, first)
        assert np.array_equal(want.reshape(-1)[-eng.L:], z["obs"][0].astype(np.float32).reshape(n_rows, -1)[-1])
        eng._check(eng.lib.rw_device_free(eng._h, out))
        env.close()


# ------------------------------------------------------------------------------------------------ CPU: the host layer
def test_host_layer_of_the_packed_format():
    lib = build_emu()
    assert _capi.load(lib).rw_abi_version() == 4 == _capi.RW_ABI_VERSION
    kw = rware_amd.env_kwargs("rware-tiny-2ag-v1")
    for ot in (rware_amd.ObservationType.IMAGE, rware_amd.ObservationType.IMAGE_DICT):
        with pytest.raises(_capi.EngineError) as ei:
            rware_amd.WarehouseVecEnv(4, library=lib, obs_format="packed", **dict(kw, observation_type=ot))
        assert ei.value.code == _capi.RW_ERR_UNSUPPORTED and "FLATTENED" in str(ei.value)
    with pytest.raises(ValueError):
        rware_amd.WarehouseVecEnv(4, library=lib, obs_format="bits", **kw)
    # without the flag: RW_BUF_OBS_PACKED is empty and everything else is as before
    env = rware_amd.make_vec("rware-tiny-2ag-v1", 4, library=lib)
    eng = env.engines[0]
    assert eng.info.obs_packed == 0 and not eng.packed
    ptr, nb = C.c_void_p(1), C.c_size_t(1)
    assert eng.lib.rw_get_buffer(eng._h, _capi.BUF["obs_packed"], C.byref(ptr), C.byref(nb)) == 0 and nb.value == 0 and not ptr.value
    assert eng.lib.rw_get_buffer(eng._h, _capi.BUF["obs"], C.byref(ptr), C.byref(nb)) == 0 and nb.value == 4 * 2 * 71 * 4 and ptr.value
    assert env.reset(seed=1)[0].dtype == np.float32 and env.observation_space.dtype == np.float32
    float_bytes = eng.info.engine_bytes_per_env_step
    env.close()
    # with the flag: RW_BUF_OBS is empty, rw_read and rw_read_outputs(obs) refuse it, rw_write refuses the packed rows
    env = rware_amd.make_vec("rware-tiny-2ag-v1", 4, library=lib, obs_format="packed")
    eng = env.engines[0]
    assert eng.info.obs_packed == 1 and eng.packed and eng.PW == 4 and env.packed_words == 4
    assert eng.lib.rw_get_buffer(eng._h, _capi.BUF["obs"], C.byref(ptr), C.byref(nb)) == 0 and nb.value == 0 and not ptr.value
    assert eng.lib.rw_get_buffer(eng._h, _capi.BUF["obs_packed"], C.byref(ptr), C.byref(nb)) == 0 and nb.value == 4 * 2 * 4 * 4 and ptr.value
    buf = np.zeros(4 * 2 * 71, np.float32)
    assert eng.lib.rw_read(eng._h, _capi.BUF["obs"], buf.ctypes.data, 0) == _capi.RW_ERR_UNSUPPORTED
    assert eng.lib.rw_read(eng._h, _capi.BUF["obs"], buf.ctypes.data, buf.nbytes) == _capi.RW_ERR_UNSUPPORTED
    assert b"RW_BUF_OBS_PACKED" in eng.lib.rw_last_error(eng._h)
    assert eng.lib.rw_read_outputs(eng._h, buf.ctypes.data, None, None, None) == _capi.RW_ERR_UNSUPPORTED
    words = np.zeros(4 * 2 * 4, np.uint32)
    assert eng.lib.rw_write(eng._h, _capi.BUF["obs_packed"], words.ctypes.data, words.nbytes) == _capi.RW_ERR_INVALID_ARG
    assert b"read-only" in eng.lib.rw_last_error(eng._h)
    with pytest.raises(RuntimeError, match="packed"):
        eng.device_array("obs")
    assert env.observation_space.dtype == np.uint32 and tuple(env.observation_space.shape) == (4, 2, 4)
    assert tuple(env.single_observation_space.shape) == (2, 4) and env.single_observation_space.dtype == np.uint32
    obs, _ = env.reset(seed=1)
    assert obs.dtype == np.uint32 and obs.shape == (4, 2, 4)
    # the packed row is what the engine prices: 16 bytes per agent instead of 284
    assert float_bytes - eng.info.engine_bytes_per_env_step == 2 * (71 - 4) * 4
    with pytest.raises(ValueError, match="unpack"):
        env.dict_from_flat(obs)
    assert env.dict_from_flat(env.unpack_obs(obs))["self"]["location"].shape == (4, 2, 2)
    env.close()
    # RW_PIPE_ON | RW_OBS_PACKED: the classic kernel, and the log says so
    env = rware_amd.make_vec("rware-small-4ag-v1", 32, library=lib, obs_format="packed", pipe=True)
    assert env.engines[0].info.pipe_workgroups == 0 and "packed" in env.engines[0].jit_log()
    env.close()
    with pytest.raises(ValueError, match="FLATTENED"):
        rware_amd.WarehouseVecEnv(4, library=lib, obs_format="packed", **dict(kw, observation_type=rware_amd.ObservationType.DICT))


def test_packed_runtime_builds_compile_without_a_device_and_get_their_own_cache_file(tmp_path, monkeypatch):
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("no hipRTC on this box")
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    shapes = [dict(sensor_range=1, H=20, W=10, N=4, Q=4, S=80, E=16),                 # rware-small-4ag (the headline)
              dict(sensor_range=2, H=29, W=16, N=16, Q=16, S=240, E=4),               # BASELINE config 5's shape
              dict(sensor_range=1, H=20, W=10, N=4, Q=4, S=80, E=16, msg_bits=2, obs=2)]
    for k, sh in enumerate(shapes):
        n1, log1 = _capi.jit_probe(packed=1, **sh)
        assert n1 > 10000 and "compiled in" in log1, log1
        n0, log0 = _capi.jit_probe(packed=0, **sh)
        assert n0 > 10000 and "compiled in" in log0, log0     # not a cache hit: the switch is part of the key
        f1, f0 = log1.split("-> ")[1].strip(), log0.split("-> ")[1].strip()
        assert f1 != f0 and os.path.exists(f1) and os.path.exists(f0)
        assert _capi.jit_probe(packed=1, **sh)[1] == "loaded " + f1
        assert len(list(tmp_path.glob("*.hsaco"))) == 2 * (k + 1)


# ------------------------------------------------------------------------------------------------ CPU: the ahead-of-time ISA guard
def test_ahead_of_time_kernels_keep_the_parent_commits_isa(tmp_path):
    """The packed rows exist only behind RW_PACKED_BUILD (generic kernels, run-time builds): the ~100 ahead-of-time exact-shape
    kernels must come out instruction for instruction as before.  tests/golden/isa/static_parent.json holds, per rware_step_kernel
    instantiation of table groups 0 (the BASELINE shapes, the headline among them) and 3, the instruction count, a hash of the opcode
    sequence and the register / LDS / scratch figures of the commit before this feature (profiles/tools/isa_stats.py with
    RWARE_ISA_JSON, run on a worktree of that commit).  The guard, not the proof of the feature: it passes on that commit too."""
    if not os.path.exists(isa_stats.HIPCC) or not shutil.which("c++filt"):
        pytest.skip("no hipcc / c++filt on this box")
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "isa", "static_parent.json")))
    ver = isa_stats.hipcc_version()
    if ver != rec["hipcc"]:
        pytest.skip(f"the figures were recorded with another hipcc:\n{rec['hipcc']}\nthis box has:\n{ver}")
    got = {}
    for g, path in isa_stats.listings(str(tmp_path), rec["groups"]).items():
        got.update({f"g{g} {k}": v for k, v in isa_stats.fingerprints(open(path).read()).items()})
    assert len(rec["kernels"]) > 20 and set(got) == set(rec["kernels"])
    diff = {k: (rec["kernels"][k], got[k]) for k in got if got[k] != rec["kernels"][k]}
    assert not diff, f"{len(diff)} ahead-of-time kernels changed: {list(diff.items())[:3]}"


# ------------------------------------------------------------------------------------------------ GPU
def _gpu_unpack(env, packed_t, out=None):
    """rw_unpack_obs on the device: packed rows (an int32 CUDA tensor (..., PW)) -> float32 (..., L)."""
    import torch
    eng = env.engines[0]
    rows = packed_t.numel() // eng.PW
    if out is None:
        out = torch.empty(tuple(packed_t.shape[:-1]) + (eng.L,), dtype=torch.float32, device=packed_t.device)
    eng.unpack_obs_device(packed_t.data_ptr(), out.data_ptr(), rows)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [False, "force"])
@pytest.mark.parametrize("name", FLAT)
def test_gpu_packed_engine_replays_reference_golden(name, jit, tmp_path, monkeypatch):
    """Every FLATTENED golden in full: on the generic kernel, and (jit="force") on the run-time exact-shape packed build — the
    fixtures hold 2 .. 4 envs, the exact-shape builds want whole workgroups: tiled, as the exact-shape tests of the float format do."""
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    meta, z = gu.load_fixture(name)
    tile = 16 if jit else 1
    be = PackedBackend(meta["E"], tile=tile, jit=jit, **gu.ctor_kwargs(meta))
    info = be.env.engines[0].info
    if jit:
        assert info.jit in (1, 2) and info.build_kind == 1, be.env.engines[0].jit_log()
    else:
        assert info.jit == 0 and info.build_kind == 0
    assert info.obs_packed == 1
    assert gu.replay(be, meta, z) == meta["T"]
    be.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,extra,B", [
    ("rware-tiny-2ag-v1", {}, 4096),                             # BASELINE config 2
    ("rware-small-4ag-v1", {}, 16384),                           # config 3 (the headline)
    ("rware-medium-6ag-hard-v1", {}, 8192),                      # config 4, per-GPU shard of 65536 / 8
    ("rware-large-16ag-v1", {"sensor_range": 2}, 16384),         # config 5, per-GPU shard of 131072 / 8
])
def test_gpu_packed_baseline_configs_every_env_every_step_against_oracle(env_id, extra, B, tmp_path, monkeypatch):
    """200 steps at the per-GPU batch: rw_unpack_obs on the device, then every env's observation (its exact checksum, taken on the
    device: tests/oracle_shards.py), rewards and flags against the oracle at every step."""
    import torch
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    kw = dict(rware_amd.env_kwargs(env_id), **extra)
    N = kw["n_agents"]
    env = rware_amd.WarehouseVecEnv(B, output="torch", obs_format="packed", **kw)
    eng = env.engines[0]
    assert eng.info.obs_packed == 1 and eng.info.jit in (1, 2) and eng.info.build_kind == 1, eng.jit_log()   # >= 4096 envs: the run-time build
    twin = rware_amd.WarehouseVecEnv(B, output="torch", **kw)   # ... on the geometry its float32 twin's ahead-of-time build runs on
    assert eng.info.envs_per_workgroup == twin.engines[0].info.envs_per_workgroup and twin.engines[0].info.jit == 0
    assert eng.info.threads_per_workgroup == twin.engines[0].info.threads_per_workgroup
    twin.close()
    orc = ShardedOracle(B, 16, **dict(kw, reward_type=kw["reward_type"].value))
    w = torch.as_tensor(orc.w, device="cuda")
    buf = torch.empty((B, N, eng.L), dtype=torch.float32, device="cuda")

    def cs(packed):
        assert packed.dtype == torch.int32 and tuple(packed.shape) == (B, N, eng.PW)
        return (_gpu_unpack(env, packed, buf).reshape(B, -1).double() @ w).cpu().numpy()

    obs, _ = env.reset(seed=77)
    assert np.array_equal(cs(obs), orc.reset(77))
    rng = np.random.default_rng(5)
    for t in range(200):
        a = rng.choice(5, size=(B, N), p=[.1, .5, .15, .15, .1]).astype(np.int32)
        obs, rew, term, _, _ = env.step(torch.as_tensor(a, device="cuda"))
        c2, r2, d2 = orc.step(a)
        assert np.array_equal(cs(obs), c2), t
        assert np.array_equal(rew.cpu().numpy(), r2) and np.array_equal(term.cpu().numpy(), d2.astype(bool)), t
    # ... and one step in full, element by element, through both unpackers
    full = _gpu_unpack(env, obs)
    assert torch.equal(full, env.unpack_obs(obs))
    o2 = np.concatenate([p.obs() for p in orc.parts])
    assert np.array_equal(full.cpu().numpy(), o2)
    env.sync()
    orc.close(); env.close()


@pytest.mark.gpu
def test_gpu_packed_262144_envs_never_hold_the_float_batch(tmp_path, monkeypatch):
    """small-4ag x 262144: 298 MB of float32 observations per step that are neither streamed nor allocated — the packed rows are
    16.8 MB.  20 steps beside float32 engines of 16384 envs each that cover the WHOLE batch between them (slice k seeded seed + lo_k: the same
    streams), every slice of every step compared through rw_unpack_obs into one slice-sized buffer."""
    import torch
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    B, N, S = 262144, 4, 16384
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    env = rware_amd.WarehouseVecEnv(B, output="torch", obs_format="packed", **kw)
    eng = env.engines[0]
    with pytest.raises(RuntimeError):
        env.device_tensor("obs")
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert eng.lib.rw_get_buffer(eng._h, _capi.BUF["obs"], C.byref(ptr), C.byref(nb)) == 0 and nb.value == 0
    slices = list(range(0, B, S))
    refs = [rware_amd.WarehouseVecEnv(S, output="torch", **kw) for _ in slices]   # float32 engines, one per slice: all 262144 envs
    packed, _ = env.reset(seed=11)
    for r, lo in zip(refs, slices):
        r.reset(seed=11 + lo)
    buf = torch.empty((S, N, eng.L), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    for t in range(20):
        a = torch.randint(0, 5, (B, N), dtype=torch.int32, device="cuda", generator=g)
        packed, rew, term, _, _ = env.step(a)
        for r, lo in zip(refs, slices):
            o, rr, tt, _, _ = r.step(a[lo:lo + S])
            assert torch.equal(_gpu_unpack(env, packed[lo:lo + S], buf), o), (t, lo)
            assert torch.equal(rew[lo:lo + S], rr) and torch.equal(term[lo:lo + S], tt), (t, lo)
    # every slice of the last step through rw_unpack_obs against the torch unpack of the same rows
    for lo in range(0, B, S):
        assert torch.equal(_gpu_unpack(env, packed[lo:lo + S], buf), env.unpack_obs(packed[lo:lo + S])), lo
    env.sync()
    for r in refs:
        r.close()
    env.close()


@pytest.mark.gpu
def test_gpu_packed_rollout_graph_pipelines_and_zero_copy(tmp_path, monkeypatch):
    """The other launch forms with packed output, each against a float32 engine run with the same seed and actions: the fused 64-step
    rollout, a HIP-graph capture of per-step launches, make_pipelines(B, 2), and the zero-copy torch tensors."""
    import torch
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    B, N, T = 4096, 4, 64
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        env = rware_amd.WarehouseVecEnv(B, output="torch", obs_format="packed", **kw)
        ref = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
        eng = env.engines[0]
        p0, _ = env.reset(seed=31)
        f0, _ = ref.reset(seed=31)
        # zero-copy: the same tensor object every step, int32 bits of the uint32 rows, unpacked on the device by plain torch ops
        assert p0.dtype == torch.int32 and p0.data_ptr() == env.device_tensor("obs_packed").data_ptr()
        assert torch.equal(env.unpack_obs(p0), f0)
        tape = torch.randint(0, 5, (T, B, N), dtype=torch.int32, device="cuda")
        # the fused 64-step rollout: obs tape (T, B, N, PW)
        otape, rew, term = env.rollout(tape)
        rtape, rrew, rterm = ref.rollout(tape)
        assert otape.dtype == torch.int32 and tuple(otape.shape) == (T, B, N, eng.PW)
        assert torch.equal(_gpu_unpack(env, otape), rtape) and torch.equal(rew, rrew) and torch.equal(term, rterm)   # one call unpacks the tape
        assert torch.equal(env.unpack_obs(otape[-1]), rtape[-1])
        # a caller's tape that starts off a 16-byte boundary (a slice of a larger buffer): the run-time build checks the pointer of a
        # fused rollout and takes the scalar stores — same rows, nothing written outside them
        assert eng.info.jit in (1, 2)
        env.reset(seed=31)
        words = T * B * N * eng.PW
        big = torch.full((words + 8,), -7, dtype=torch.int32, device="cuda")
        eng.step_many_device(tape.data_ptr(), T, obs_tape=big.data_ptr() + 4)
        assert torch.equal(big[1:1 + words].view(T, B, N, eng.PW), otape)
        assert int(big[0]) == -7 and bool((big[1 + words:] == -7).all())
        # a HIP graph of per-step launches
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            eng.step_tape_device(tape.data_ptr(), T, 0, T)
        g.replay()
        for t in range(T):
            ref.engines[0].step_device(tape[t].data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(env.unpack_obs(env.device_tensor("obs_packed")), ref.device_tensor("obs"))
        assert torch.equal(env.device_tensor("rewards"), ref.device_tensor("rewards"))
    a, b = env.get_state(), ref.get_state()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    env.close()
    # two pipelines of half the batch each, packed, against the whole float32 batch
    pipes = rware_amd.make_pipelines(B, 2, env_id="rware-small-4ag-v1", obs_format="packed")
    with torch.cuda.stream(s):
        f, _ = ref.reset(seed=5)
    for p in pipes:
        o, _ = p.reset(seed=5)
        with p as e:
            assert e.engines[0].info.obs_packed == 1 and o.dtype == torch.int32
    for t in range(10):
        with torch.cuda.stream(s):
            f, fr, ft, _, _ = ref.step(tape[t])
        torch.cuda.synchronize()
        for p in pipes:
            with p as e:
                o, r, d, _, _ = e.step(tape[t, p.lo:p.hi].contiguous())
                p.stream.synchronize()
                assert torch.equal(e.unpack_obs(o), f[p.lo:p.hi]) and torch.equal(r, fr[p.lo:p.hi]) and torch.equal(d, ft[p.lo:p.hi]), t
    for p in pipes:
        p.env.close()
    ref.close()
