"""uint8 IMAGE observations (obs_format="uint8", RW_OBS_IMAGE_U8): the emulated engine against every image golden trace and against
the oracle on the shapes whose chunks start off a 16-byte boundary, the other launch forms, the host layer, the run-time builds and
the guard on the ahead-of-time image kernels' ISA; on a GPU the generic kernel, the run-time exact-shape uint8 build, the torch and
captured forms.

The reference in every comparison is the float32 image of the golden fixtures (recorded from the unmodified reference) or of the
oracle; every comparison is exact, by value (a uint8 element against the float32 element it stands for), and everything the engine
hands out is checked to BE uint8."""
import ctypes as C
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

import golden_util as gu
import lockstep as ls
from engine_backend import EngineBackend, build_emu
from rware_oracle import OracleVecEnv

import rware_amd
from rware_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "profiles", "tools", "isa_stats.py"))
isa_stats = importlib.util.module_from_spec(_spec)      # the tool that recorded tests/golden/isa/*.json: its compile and its figures
_spec.loader.exec_module(isa_stats)
pytestmark = pytest.mark.timeout(1500)
P_ACT = [.1, .5, .15, .15, .1]


def _image_goldens():
    names = []
    for n in gu.fixture_names():
        meta, _ = gu.load_fixture(n)
        if int(meta["kwargs"].get("observation_type", 1) or 1) in (2, 3):   # IMAGE, IMAGE_DICT
            names.append(n)
    return names


IMG = _image_goldens()
# the shapes where the stores can go wrong: bytes per agent 27 (a 4-env chunk of 5 agents is 540 bytes — chunk 1 starts 12 bytes past a
# 16-byte boundary; the last chunk of 7 envs holds 405 bytes, an odd count), 63 (aligned chunks; the last one 756 bytes, whole dwords
# but no whole 16-byte pieces at its end), 200 (everything aligned, sensor_range 2)
ALIGN = ["imgdict-square-5ag-transposed-northup", "img-square-all7-msg1", "img-msg2-tiny-3ag-8layers"]
GEOMS = [((4, 64), 7), ((16, 256), 40)]


def _u8(o):
    """The image part of what the engine handed out — and it is uint8 (IMAGE_DICT: the features stay float32)."""
    if isinstance(o, dict):
        assert o["features"].dtype == np.float32, o["features"].dtype
        o = o["image"]
    assert o.dtype == np.uint8, o.dtype
    return o


class U8Backend(EngineBackend):
    """The replay harness's adapter over an obs_format="uint8" env: asserts the dtype of every observation and counts them;
    golden_util.replay then compares the values with the fixture's float32 image, exactly."""

    def __init__(self, *a, **kw):
        super().__init__(*a, obs_format="uint8", **kw)
        self.n_obs = 0

    def _obs(self, o):
        _u8(o)
        self.n_obs += 1
        return super()._obs(o)


def _shape_kwargs(name, **extra):
    meta, _ = gu.load_fixture(name)
    return dict(gu.ctor_kwargs(meta), **extra)


def _draw(rng, kw, *lead):
    a = rng.choice(5, size=lead + (kw["n_agents"],), p=P_ACT).astype(np.int32)
    if kw.get("msg_bits", 0):
        a = np.concatenate([a[..., None], rng.integers(0, 2, size=a.shape + (kw["msg_bits"],)).astype(np.int32)], axis=-1)
    return a


def _lockstep_u8(env, orc, kw, B, mode, steps, seed=5):
    """lockstep() with the dtype of every observation asserted; autoreset disabled: the ended envs are reset by mask (a masked rw_reset)."""
    rng = np.random.default_rng(1)
    seen = {"n": 0}

    def on_step(t, obs, rew, term, info):
        _u8(obs)
        seen["n"] += 1
        if "final_obs" in info:   # the terminal observation stays float32
            f = info["final_obs"]
            assert (f["image"] if isinstance(f, dict) else f).dtype == np.float32
        if mode == "disabled" and term.any():
            m = term.astype(np.uint8)
            o = env.reset(mask=m)[0]
            _u8(o)
            ls.same_obs(o, orc.reset(mask=m), "masked reset obs", t)

    _u8(env.reset(seed=seed)[0])
    run = ls.lockstep(env, orc, lambda t: _draw(rng, kw, B), mode, seed=seed, steps=steps, on_step=on_step)
    assert seen["n"] == steps
    return run


# ------------------------------------------------------------------------------------------------ CPU: the emulated engine
def test_there_are_seven_image_goldens():
    assert len(IMG) == 7, IMG
    assert set(ALIGN) <= set(IMG) and sum(n.startswith("imgdict-") for n in IMG) == 2


@pytest.mark.parametrize("name", IMG)
def test_emulated_uint8_engine_replays_reference_golden(name):
    meta, z = gu.load_fixture(name)
    be = U8Backend(meta["E"], library=build_emu(), **gu.ctor_kwargs(meta))
    info = be.env.engines[0].info
    assert info.obs_packed == 2 and info.build_kind == 0      # uint8 rows: never an ahead-of-time specialised build
    assert ("features" in z) == name.startswith("imgdict-")   # (replay compares the IMAGE_DICT features as well)
    assert gu.replay(be, meta, z, steps=120) == min(120, meta["T"]) and be.n_obs > 1
    be.env.close()


@pytest.mark.parametrize("geom,B", GEOMS)
@pytest.mark.parametrize("mode", ["next_step", "same_step", "disabled"])
@pytest.mark.parametrize("name", ALIGN)
def test_emulated_uint8_alignment_cases_match_oracle(name, mode, geom, B):
    kw = _shape_kwargs(name, max_steps=12)
    env = rware_amd.WarehouseVecEnv(B, library=build_emu(), autoreset_mode=mode, obs_format="uint8", envs_per_workgroup=geom[0],
                                    threads_per_workgroup=geom[1], **kw)
    eng = env.engines[0]
    assert eng.info.obs_packed == 2 and eng.info.envs_per_workgroup == geom[0] and eng.info.threads_per_workgroup == geom[1]
    assert eng.L == {ALIGN[0]: 27, ALIGN[1]: 63, ALIGN[2]: 200}[name]
    orc = OracleVecEnv(B, **kw)
    run = _lockstep_u8(env, orc, kw, B, mode, steps=30)
    assert run.episodes > 0 and (mode != "same_step" or run.finals > 0)
    env.close()


@pytest.mark.parametrize("offset", [1, 4])
def test_emulated_fused_rollout_into_a_callers_tape_at_any_byte_address(offset):
    """rw_step_many_device with `obs_tape` 1 and 4 bytes past a 16-byte boundary, 27 bytes per agent, 7 envs of 5 agents on 4-env
    workgroups: step k starts k * 945 bytes further on — every alignment class occurs.  Every step equals a float32 twin engine
    stepped on the same actions, and the allocated bytes in front of and behind the tape keep their pattern."""
    kw = _shape_kwargs(ALIGN[0], max_steps=7)
    B, T, N = 7, 9, kw["n_agents"]
    geom = dict(envs_per_workgroup=4, threads_per_workgroup=64)
    env = rware_amd.WarehouseVecEnv(B, library=build_emu(), obs_format="uint8", **geom, **kw)
    ref = rware_amd.WarehouseVecEnv(B, library=build_emu(), **geom, **kw)
    env.reset(seed=3); ref.reset(seed=3)
    acts = np.ascontiguousarray(_draw(np.random.default_rng(2), kw, T, B))
    eng = env.engines[0]
    assert eng.L == 27 and eng.image_u8
    n = T * B * N * eng.L
    PAD = 64
    d_a, d_o = C.c_void_p(), C.c_void_p()
    eng._check(eng.lib.rw_device_malloc(eng._h, acts.nbytes, C.byref(d_a)))
    eng._check(eng.lib.rw_device_malloc(eng._h, PAD + offset + n + PAD, C.byref(d_o)))
    assert d_o.value % 16 == 0
    eng._check(eng.lib.rw_copy_to_device(eng._h, d_a, acts.ctypes.data, acts.nbytes))
    pattern = (np.arange(PAD + offset + n + PAD) * 7 + 0xA5).astype(np.uint8)
    eng._check(eng.lib.rw_copy_to_device(eng._h, d_o, pattern.ctypes.data, pattern.nbytes))
    eng.step_many_device(d_a.value, T, obs_tape=d_o.value + PAD + offset)
    back = np.zeros_like(pattern)
    eng._check(eng.lib.rw_copy_to_host(eng._h, back.ctypes.data, d_o, back.nbytes))
    lo, hi = PAD + offset, PAD + offset + n
    assert np.array_equal(back[:lo], pattern[:lo]) and np.array_equal(back[hi:], pattern[hi:]), "bytes outside the tape were written"
    tape = back[lo:hi].reshape((T,) + eng.shapes["obs"])
    for t in range(T):
        want = ref.step(acts[t])[0]
        assert want["image"].dtype == np.float32 and np.array_equal(tape[t], want["image"]), t
    eng._check(eng.lib.rw_device_free(eng._h, d_a)); eng._check(eng.lib.rw_device_free(eng._h, d_o))
    # ... and through the Python surface: rollout() returns a uint8 tape
    env.reset(seed=3); ref.reset(seed=3)
    otape, rew, term = env.rollout(acts)
    rtape, rrew, rterm = ref.rollout(acts)
    assert otape.dtype == np.uint8 and rtape.dtype == np.float32 and otape.shape == rtape.shape == (T,) + eng.shapes["obs"]
    assert np.array_equal(otape, rtape) and np.array_equal(rew, rrew) and np.array_equal(term, rterm)
    env.close(); ref.close()


def test_emulated_refresh_restore_and_masked_reset_produce_uint8_rows():
    kw = _shape_kwargs(ALIGN[0], max_steps=9)
    B = 10
    env = rware_amd.WarehouseVecEnv(B, library=build_emu(), obs_format="uint8", **kw)
    ref = rware_amd.WarehouseVecEnv(B, library=build_emu(), **kw)
    env.reset(seed=8); ref.reset(seed=8)
    rng = np.random.default_rng(4)
    for t in range(6):
        a = _draw(rng, kw, B)
        ls.same_obs(env.step(a)[0], tuple(ref.step(a)[0].values()), "obs", t)
    # rw_refresh_obs after set_state: the uint8 rows follow the injected state
    st = ref.get_state()
    tok = env.snapshot()
    env.reset(seed=99)
    assert not np.array_equal(env.observations()["image"], ref.observations()["image"])
    env.set_state(**{k: st[k] for k in st})
    ls.same_obs({"image": _u8(env.observations()), "features": env.observations()["features"]}, tuple(ref.observations().values()), "refreshed obs")
    # rw_snapshot_restore recomputes the observation in the engine's format
    env.reset(seed=99)
    o = env.restore(tok)
    ls.same_obs({"image": _u8(o), "features": o["features"]}, tuple(ref.observations().values()), "restored obs")
    env.free_snapshot(tok)
    # a masked rw_reset: the masked envs get a fresh uint8 observation, the others keep theirs
    m = (np.arange(B) % 3 == 0).astype(np.uint8)
    o, r = env.reset(seed=50, mask=m)[0], ref.reset(seed=50, mask=m)[0]
    ls.same_obs({"image": _u8(o), "features": o["features"]}, tuple(r.values()), "masked reset obs")
    env.close(); ref.close()


def test_emulated_uint8_image_dict_with_every_side_output_matches_oracle():
    kw = _shape_kwargs(ALIGN[0], max_steps=12)
    B = 9
    side = dict(stats=True, episode_stats=True, action_mask=True, envs_per_workgroup=4, threads_per_workgroup=128)
    env = rware_amd.WarehouseVecEnv(B, library=build_emu(), obs_format="uint8", **side, **kw)
    ref = rware_amd.WarehouseVecEnv(B, library=build_emu(), **side, **kw)
    assert env.engines[0].info.stats == 7 and env.engines[0].info.obs_packed == 2 and ref.engines[0].info.obs_packed == 0
    orc = OracleVecEnv(B, **kw)
    ref.reset(seed=5)
    rng = np.random.default_rng(1)
    acts = _draw(rng, kw, 30, B)

    def twin(t, obs, rew, term, info):
        _u8(obs)
        ref.step(acts[t])
        assert np.array_equal(info["action_mask"], ref.action_mask()), t

    run = ls.lockstep(env, orc, acts, seed=5, on_step=twin)
    assert run.episodes >= B
    for got, want in ((env.event_counters(), ref.event_counters()), (env.episode_stats(), ref.episode_stats())):
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    assert env.episode_stats()["count"].sum() == run.episodes and env.event_counters()["failed_moves"].sum() > 0
    assert np.array_equal(env.action_mask(), ref.action_mask())
    env.close(); ref.close()


# ------------------------------------------------------------------------------------------------ CPU: the host layer
def test_host_layer_of_the_uint8_format():
    lib = build_emu()
    assert _capi.load(lib).rw_abi_version() == 4 == _capi.RW_ABI_VERSION
    assert _capi.RW_OBS_IMAGE_U8 == 8192 and len(_capi.BUFFERS) == 29 and _capi.BUF_DTYPE["obs"] == np.float32
    flat = rware_amd.env_kwargs("rware-tiny-2ag-v1")
    # the refusals: FLATTENED (Python names the IMAGE types, and so does the engine), DICT, together with RW_OBS_PACKED
    for ot in (rware_amd.ObservationType.FLATTENED, rware_amd.ObservationType.DICT):
        with pytest.raises(ValueError, match="IMAGE"):
            rware_amd.WarehouseVecEnv(4, library=lib, obs_format="uint8", **dict(flat, observation_type=ot))
    with pytest.raises(ValueError):
        rware_amd.WarehouseVecEnv(4, library=lib, obs_format="u8", **flat)
    lay = rware_amd.layout_from_params(3, 1, 8)
    cfg = dict(num_envs=4, layout=lay, n_agents=2, sensor_range=1, request_queue_size=2, max_inactivity_steps=None, max_steps=500,
               reward_type=1, library=lib)
    with pytest.raises(_capi.EngineError) as ei:
        _capi.Engine(observation_type=1, obs_image_u8=True, **cfg)
    assert ei.value.code == _capi.RW_ERR_UNSUPPORTED and "IMAGE" in str(ei.value)
    for ot in (2, 3):
        with pytest.raises(_capi.EngineError) as ei:
            _capi.Engine(observation_type=ot, obs_image_u8=True, obs_packed=True, **cfg)
        assert ei.value.code == _capi.RW_ERR_UNSUPPORTED
    # a float32 IMAGE engine and its uint8 twin
    kw = dict(flat, observation_type=rware_amd.ObservationType.IMAGE)
    env = rware_amd.WarehouseVecEnv(4, library=lib, **kw)
    assert env.engines[0].info.obs_packed == 0 and env.reset(seed=1)[0].dtype == np.float32 and env.observation_space.dtype == np.float32
    float_bytes, float_obs = env.engines[0].info.engine_bytes_per_env_step, env.observations()
    env.close()
    env = rware_amd.WarehouseVecEnv(4, library=lib, obs_format="uint8", **kw)
    eng = env.engines[0]
    N, L = 2, 45
    assert eng.info.obs_packed == 2 and eng.image_u8 and not eng.packed and eng.info.obs_length == L == eng.L
    assert eng.dtypes["obs"] == np.uint8 and eng.shapes["obs"] == (4, N, 5, 3, 3) and eng.obs_name == "obs"
    ptr, dptr, nb = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert eng.lib.rw_get_buffer(eng._h, _capi.BUF["obs"], C.byref(dptr), C.byref(nb)) == 0 and nb.value == 4 * N * L and dptr.value
    assert eng.lib.rw_get_buffer(eng._h, _capi.BUF["obs_packed"], C.byref(ptr), C.byref(nb)) == 0 and nb.value == 0 and not ptr.value
    obs, _ = env.reset(seed=1)
    assert obs.dtype == np.uint8 and np.array_equal(obs, float_obs) and obs.max() <= 4
    buf = np.zeros(4 * N * L, np.float32)
    assert eng.lib.rw_read(eng._h, _capi.BUF["obs"], buf.ctypes.data, buf.nbytes) == _capi.RW_ERR_INVALID_ARG     # the float size
    b8 = np.zeros(4 * N * L, np.uint8)
    assert eng.lib.rw_read(eng._h, _capi.BUF["obs"], b8.ctypes.data, b8.nbytes) == 0 and np.array_equal(b8, obs.reshape(-1))
    o8 = np.full(4 * N * L + 8, 0xEE, np.uint8)      # rw_read_outputs moves B * N * L bytes through its `obs` argument
    assert eng.lib.rw_read_outputs(eng._h, o8.ctypes.data, None, None, None) == 0
    assert np.array_equal(o8[:-8], b8) and (o8[-8:] == 0xEE).all()
    assert eng.lib.rw_write(eng._h, _capi.BUF["obs"], b8.ctypes.data, b8.nbytes) == 0
    assert eng.lib.rw_write(eng._h, _capi.BUF["obs"], buf.ctypes.data, buf.nbytes) == _capi.RW_ERR_INVALID_ARG
    assert np.array_equal(eng.read("obs"), obs) and eng.read("obs").dtype == np.uint8
    assert eng.lib.rw_unpack_obs(eng._h, dptr, dptr, 1) == _capi.RW_ERR_UNSUPPORTED
    ms = C.c_float()
    assert eng.lib.rw_debug_store_floor(eng._h, 1, C.byref(ms)) == _capi.RW_ERR_UNSUPPORTED
    # the uint8 row is what the engine prices: obs_length bytes per agent instead of 4 * obs_length
    assert float_bytes - eng.info.engine_bytes_per_env_step == 3 * N * L
    # the spaces: Box(0, 4, uint8) of the image shape
    sp, one = env.observation_space, env.single_observation_space
    assert sp.dtype == np.uint8 and tuple(sp.shape) == (4, N, 5, 3, 3) and np.min(sp.low) == 0 and np.max(sp.high) == 4
    assert len(one) == N and one[0].dtype == np.uint8 and tuple(one[0].shape) == (5, 3, 3) and np.max(one[0].high) == 4
    env.close()
    # IMAGE_DICT: the image entry in uint8, the features float32 — through make_vec
    env = rware_amd.make_vec("rware-tiny-2ag-v1", 4, library=lib, obs_format="uint8", observation_type=rware_amd.ObservationType.IMAGE_DICT,
                             autoreset_mode="same_step")
    o = env.reset(seed=1)[0]
    assert _u8(o).shape == (4, N, 5, 3, 3) and o["features"].shape == (4, N, 6)
    img, feat = env.observation_space["image"], env.observation_space["features"]
    assert img.dtype == np.uint8 and tuple(img.shape) == (4, N, 5, 3, 3) and np.max(img.high) == 4 and feat.dtype == np.float32
    assert env.single_observation_space[0]["image"].dtype == np.uint8
    assert env.engines[0].read("final_obs").dtype == np.float32 and env.engines[0].read("features").dtype == np.float32
    env.close()
    # RW_PIPE_ON | RW_OBS_IMAGE_U8: the classic kernel, and the log says so
    env = rware_amd.make_vec("rware-small-4ag-v1", 32, library=lib, obs_format="uint8", observation_type=rware_amd.ObservationType.IMAGE, pipe=True)
    assert env.engines[0].info.pipe_workgroups == 0 and "RW_OBS_IMAGE_U8" in env.engines[0].jit_log()
    env.close()
    # RW_OBS_PACKED with an IMAGE type keeps failing as before
    with pytest.raises(_capi.EngineError) as ei:
        rware_amd.WarehouseVecEnv(4, library=lib, obs_format="packed", **kw)
    assert ei.value.code == _capi.RW_ERR_UNSUPPORTED and "FLATTENED" in str(ei.value)


def test_uint8_runtime_builds_compile_without_a_device_and_get_their_own_cache_file(tmp_path, monkeypatch):
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("no hipRTC on this box")
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    shapes = [dict(sensor_range=1, H=20, W=10, N=4, Q=4, S=80, E=16, obs=1, layers=(0, 1, 2, 5, 6)),                  # rware-small-4ag, the default layers
              dict(sensor_range=1, H=10, W=10, N=5, Q=3, S=36, E=4, obs=1, layers=(4, 5, 3), directional=False)]      # 27 bytes per agent, AGENT_DIRECTION
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
def test_ahead_of_time_image_kernels_keep_the_parent_commits_isa(tmp_path):
    """The uint8 rows exist only behind RW_PACKED_BUILD (generic kernels, run-time builds): the ahead-of-time image builds — table
    group 1 — must come out instruction for instruction as before.  tests/golden/isa/static_image_parent.json holds their figures
    from the commit before this feature (profiles/tools/isa_stats.py with RWARE_ISA_JSON, run on a worktree of that commit), as
    static_parent.json does for groups 0 and 3.  A guard, not the proof of the feature: it passes on that commit too."""
    if not os.path.exists(isa_stats.HIPCC) or not shutil.which("c++filt"):
        pytest.skip("no hipcc / c++filt on this box")
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "isa", "static_image_parent.json")))
    ver = isa_stats.hipcc_version()
    if ver != rec["hipcc"]:
        pytest.skip(f"the figures were recorded with another hipcc:\n{rec['hipcc']}\nthis box has:\n{ver}")
    assert rec["groups"] == [1]
    got = {f"g1 {k}": v for k, v in isa_stats.fingerprints(open(isa_stats.listings(str(tmp_path), [1])[1]).read()).items()}
    image = [k for k in got if k.rstrip(">").endswith(", 1")]     # (kObs == OBS_IMAGE, the last template argument)
    assert len(rec["kernels"]) >= 6 and image and set(got) == set(rec["kernels"])
    diff = {k: (rec["kernels"][k], got[k]) for k in got if got[k] != rec["kernels"][k]}
    assert not diff, f"{len(diff)} ahead-of-time kernels changed: {list(diff.items())[:3]}"


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("jit", [False, "force"])
@pytest.mark.parametrize("name", IMG)
def test_gpu_uint8_engine_replays_reference_golden(name, jit, tmp_path, monkeypatch):
    """Every image golden in full: on the generic kernel, and (jit="force") on the run-time exact-shape uint8 build — the fixtures
    hold 2 .. 3 envs, the exact-shape builds want whole workgroups: tiled, as the exact-shape tests of the float format do."""
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    meta, z = gu.load_fixture(name)
    be = U8Backend(meta["E"], tile=16 if jit else 1, jit=jit, **gu.ctor_kwargs(meta))
    info = be.env.engines[0].info
    if jit:
        assert info.jit in (1, 2) and info.build_kind == 1, be.env.engines[0].jit_log()
    else:
        assert info.jit == 0 and info.build_kind == 0
    assert info.obs_packed == 2
    assert gu.replay(be, meta, z) == meta["T"]
    be.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geom,B", GEOMS)
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
@pytest.mark.parametrize("name", ALIGN)
def test_gpu_uint8_alignment_cases_match_oracle(name, mode, geom, B):
    kw = _shape_kwargs(name, max_steps=12)
    env = rware_amd.WarehouseVecEnv(B, autoreset_mode=mode, obs_format="uint8", envs_per_workgroup=geom[0], threads_per_workgroup=geom[1], **kw)
    assert env.engines[0].info.obs_packed == 2 and env.engines[0].info.build_kind == 0
    run = _lockstep_u8(env, OracleVecEnv(B, **kw), kw, B, mode, steps=40)
    assert run.episodes > 0 and (mode != "same_step" or run.finals > 0)
    env.close()


class _TorchAsNumpy:
    """An output="torch" env behind the numpy surface lockstep() and check_rollout() drive: every observation it hands on was a
    torch.uint8 CUDA tensor; rollout() goes through the device path (a CUDA action tape in, a torch uint8 tape out)."""

    def __init__(self, env):
        import torch
        self.env, self.torch = env, torch

    def _obs(self, o):
        assert o.is_cuda and o.dtype == self.torch.uint8, o.dtype
        return o.cpu().numpy()

    def reset(self, seed=None):
        return self._obs(self.env.reset(seed=seed)[0]), {}

    def step(self, a):
        o, r, d, tr, info = self.env.step(self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda"))
        return self._obs(o), r.cpu().numpy(), d.cpu().numpy(), tr.cpu().numpy(), info

    def rollout(self, acts):
        tape, rew, term = self.env.rollout(self.torch.as_tensor(np.ascontiguousarray(acts, dtype=np.int32), device="cuda"))
        assert tape.dtype == self.torch.uint8 and tape.is_cuda
        return tape.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy()

    def get_state(self):
        return self.env.get_state()


@pytest.mark.gpu
def test_gpu_uint8_default_runtime_build_every_env_every_step_against_oracle(tmp_path, monkeypatch):
    """rware-small-4ag IMAGE, the default layers, x 4096: rw_create's default rule compiles the exact-shape uint8 build.  60 steps, every
    env, every step against the oracle; then a 16-step fused rollout into a torch uint8 tape."""
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    B = 4096
    kw = ls.oracle_kwargs("rware-small-4ag-v1", observation_type=2, max_steps=40)
    env = rware_amd.WarehouseVecEnv(B, output="torch", obs_format="uint8", **kw)
    eng = env.engines[0]
    assert eng.info.obs_packed == 2 and eng.info.jit in (1, 2) and eng.info.build_kind == 1, eng.jit_log()
    orc = OracleVecEnv(B, **kw)
    rng = np.random.default_rng(5)
    ad = _TorchAsNumpy(env)
    run = ls.lockstep(ad, orc, lambda t: _draw(rng, kw, B), seed=77, steps=60, state_every=20)
    assert run.episodes >= B
    ls.check_rollout(ad, orc, _draw(rng, kw, 16, B), t0=60)
    env.sync()
    env.close()


@pytest.mark.gpu
def test_gpu_uint8_zero_copy_captured_loop_and_pipelines(tmp_path, monkeypatch):
    """The torch forms: the zero-copy uint8 observation is current after step() without a sync on the caller's stream; a capture_loop
    replay produces the rows eager steps produce; two pipelines match the oracle."""
    import torch
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    B, N, K = 4096, 4, 12
    kw = ls.oracle_kwargs("rware-small-4ag-v1", observation_type=2, max_steps=30)
    tape_np = np.random.default_rng(3).choice(5, size=(K, B, N), p=P_ACT).astype(np.int32)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        env = rware_amd.WarehouseVecEnv(B, output="torch", obs_format="uint8", **kw)
        ref = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
        tape = torch.from_numpy(tape_np).cuda()
        o, _ = env.reset(seed=31)
        f, _ = ref.reset(seed=31)
        raw = env.device_tensor("obs")
        assert o.dtype == torch.uint8 and o.data_ptr() == raw.data_ptr() == env.engines[0].device_array("obs").ptr and tuple(o.shape) == (B, N, 5, 3, 3)
        assert f.dtype == torch.float32 and torch.equal(o.float(), f)
        eager = []
        for t in range(K):           # no sync between the step and the comparison: both are enqueued on this stream
            o2, r, d, _, _ = env.step(tape[t])
            f2, fr, fd, _, _ = ref.step(tape[t])
            assert o2.data_ptr() == raw.data_ptr() and torch.equal(o2.float(), f2) and torch.equal(r, fr) and torch.equal(d, fd), t
            eager.append(o2.clone())
        ref.close()
        env.close()
    torch.cuda.synchronize()
    # a captured loop: the policy records the observation it is shown and plays the tape
    cenv = rware_amd.WarehouseVecEnv(B, output="torch", obs_format="uint8", **kw)
    cenv.reset(seed=31)
    cursor = torch.zeros((), dtype=torch.long, device="cuda")
    record = torch.zeros((K, B, N, 5, 3, 3), dtype=torch.uint8, device="cuda")

    def policy(obs, rewards, terminated):
        assert obs.dtype == torch.uint8
        record.index_copy_(0, cursor.reshape(1), obs.unsqueeze(0))
        a = tape.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return a

    loop = cenv.capture_loop(policy, steps=K, warmup=0)
    cursor.zero_(); record.zero_()
    loop.replay()
    torch.cuda.synchronize()
    for t in range(1, K):            # record[t]: the observation in front of step t == what eager step t - 1 returned
        assert torch.equal(record[t], eager[t - 1]), t
    assert torch.equal(cenv.device_tensor("obs"), eager[K - 1])
    cenv.close()
    # two pipelines of half the batch each against the oracle
    pipes = rware_amd.make_pipelines(B, 2, obs_format="uint8", **kw)
    orc = OracleVecEnv(B, **kw)
    want = orc.reset(seed=11)
    for p in pipes:
        o, _ = p.reset(seed=11)
        p.stream.synchronize()
        assert o.dtype == torch.uint8 and np.array_equal(o.cpu().numpy(), want[p.lo:p.hi])
    for t in range(10):
        o2, r2, d2 = orc.step_autoreset(tape_np[t], "next_step")
        for p in pipes:
            with p as e:
                o, r, d, _, _ = e.step(tape[t, p.lo:p.hi].contiguous())
                p.stream.synchronize()
                assert e.engines[0].info.obs_packed == 2 and o.dtype == torch.uint8
                assert np.array_equal(o.cpu().numpy(), o2[p.lo:p.hi]) and np.array_equal(r.cpu().numpy(), r2[p.lo:p.hi]), t
                assert np.array_equal(d.cpu().numpy(), d2[p.lo:p.hi].astype(bool)), t
    for p in pipes:
        p.env.close()
