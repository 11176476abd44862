"""Per-episode return and length kept on the device (rw_stream_flags RW_EPISODES_ON; WarehouseVecEnv(episode_stats=True)).

The reference keeps no such figures (its `info` is {}), so the expected values come from a model in plain numpy — EpisodeModel below, the
contract of include/rware_hip.h at RW_EPISODES_ON — fed with each step's (rewards, terminated) from the ORACLE side of lockstep.lockstep.
The model is pinned to the reference once: the golden traces' recorded rewards and done flags go through it and through the engine.
Every lockstep run compares all five buffers after every step with array_equal (rewards are multiples of 0.5: the float32 sums are exact)
and has to finish at least two episodes on some env.
  - CPU suite: the product sources on host threads (tests/emu): every autoreset mode, generic / exact-shape / per-cell builds, the fused
    rollout (three episode ends inside one launch), masked resets, state writes, snapshots, shards, the off switch, step()'s info keys;
  - GPU suite (-m gpu): the gfx950 library — generic and run-time compiled builds, the fused rollout, zero-copy tensors under a captured loop.
"""
import numpy as np
import pytest

import golden_util as gu
import lockstep
from device_backends import emu_library
from models import EPISODE_BUFFERS, EpisodeModel, same_buffers
from rware_oracle import OracleVecEnv

import rware_amd

MODES = ["next_step", "same_step", "disabled"]
P_ACT = [.05, .7, .1, .1, .05]


def make_pair(lib, env_id, extra, B, mode, geom=(0, 0), jit=None, **env_kw):
    kw = lockstep.oracle_kwargs(env_id, **extra)
    env = rware_amd.WarehouseVecEnv(B, autoreset_mode=mode, library=lib, episode_stats=True, envs_per_workgroup=geom[0],
                                    threads_per_workgroup=geom[1], jit=jit, **env_kw, **kw)
    assert not jit or env.engines[0].info.jit in (1, 2), env.engines[0].jit_log()
    return env, OracleVecEnv(B, **kw), kw


def check_against_model(lib, env_id, extra, B, T, mode, geom=(0, 0), seed=17, jit=None, **env_kw):
    """env beside oracle (every field of the step compared by the harness), the five buffers beside the model after every step"""
    env, orc, kw = make_pair(lib, env_id, extra, B, mode, geom, jit, **env_kw)
    model = EpisodeModel(B, kw["n_agents"], mode)
    rng = np.random.default_rng(seed)
    seen = []

    class Tap:   # the oracle's (rewards, terminated) of each step, as the harness gets them
        def __getattr__(self, k):
            return getattr(orc, k)

        def step_autoreset(self, a, m):
            out = orc.step_autoreset(a, m)
            seen.append((np.array(out[1]), np.array(out[2])))
            return out

    def buffers(t, obs, rew, term, info):
        model.step(*seen[-1])
        same_buffers(env.episode_stats(), model, (mode, t))
        if np.asarray(term).any():   # (numpy output: Gymnasium's keys on the steps that finish an episode, and only there)
            assert np.array_equal(info["_episode"], np.asarray(term, bool))
            assert np.array_equal(info["episode"]["l"][info["_episode"]], model.v["last_length"][info["_episode"]])
        else:
            assert "episode" not in info and "_episode" not in info

    lockstep.lockstep(env, Tap(), lambda t: rng.choice(5, size=(B, kw["n_agents"]), p=P_ACT).astype(np.int32), mode, seed=seed, steps=T,
                      on_step=buffers)
    assert model.v["count"].max() >= 2, "the run finished fewer than two episodes on every env: it proves nothing"
    env.close()
    return model


def check_rollout(lib, env_id, extra, B, mode, geom=(0, 0), jit=None, T=30):
    """one fused launch of T steps with three episode ends inside it on every env == T single steps; three single steps carry on"""
    env, orc, kw = make_pair(lib, env_id, extra, B, mode, geom, jit)
    model = EpisodeModel(B, kw["n_agents"], mode)
    env.reset(seed=5)
    orc.reset(seed=5)
    acts = np.random.default_rng(1).choice(5, size=(T + 3, B, kw["n_agents"]), p=P_ACT).astype(np.int32)
    _, rew, term = env.rollout(acts[:T], want_obs=False)
    for t in range(T):
        _, r2, d2 = orc.step_autoreset(acts[t], mode)
        assert np.array_equal(rew[t], r2) and np.array_equal(term[t], d2.astype(bool)), t
        model.step(r2, d2)
    assert model.v["count"].min() >= 3
    same_buffers(env.episode_stats(), model, (mode, "after the rollout"))
    for t in range(T, T + 3):
        env.step(acts[t])
        model.step(*orc.step_autoreset(acts[t], mode)[1:])
        same_buffers(env.episode_stats(), model, (mode, t))
    env.close()


def replay_golden(name, lib, steps=None, **env_kw):
    """the pin to the reference: a golden trace's recorded rewards and done flags through the model, its actions through the engine"""
    meta, z = gu.load_fixture(name)
    kw = gu.ctor_kwargs(meta)
    env = rware_amd.WarehouseVecEnv(meta["E"], library=lib, episode_stats=True, **env_kw, **kw)
    model = EpisodeModel(meta["E"], kw["n_agents"], "next_step")
    env.reset(seed=meta["seed"])
    T = min(steps or meta["T"], meta["T"])
    for t in range(T):
        _, rew, term, _, _ = env.step(z["actions"][t].astype(np.int32))
        assert np.array_equal(rew, z["rewards"][t]) and np.array_equal(term, z["done"][t].astype(bool)), (name, t)
        model.step(z["rewards"][t], z["done"][t])
        same_buffers(env.episode_stats(), model, (name, t))
    env.close()
    return int(z["done"][:T].sum()), float(np.abs(z["rewards"][:T]).sum())


# ------------------------------------------------------------------------------------------------------------------------------
# CPU suite: the product sources on host threads
# ------------------------------------------------------------------------------------------------------------------------------
# (trace, steps replayed, geometry): an IMAGE trace with messages and episode ends, TWO_STAGE (0.5 rewards), GLOBAL rewards
EMU_GOLDEN = [("img-msg2-tiny-3ag-8layers", 100, {}), ("tiny-4ag-easy-twostage", 60, {"envs_per_workgroup": 4, "threads_per_workgroup": 128}),
              ("medium-2ag-easy", 160, {"envs_per_workgroup": 4, "threads_per_workgroup": 64})]


def test_the_replayed_golden_traces_contain_an_episode_end():
    ends = 0
    for name, steps, _ in EMU_GOLDEN:
        ends += int(gu.load_fixture(name)[1]["done"][:steps].sum())
    assert ends > 0 and sum(int(gu.load_fixture(n)[1]["done"].sum()) for n in gu.fixture_names()) > 0


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("name,steps,geom", EMU_GOLDEN)
def test_emulated_engine_and_model_agree_on_the_references_traces(name, steps, geom):
    ends, rew = replay_golden(name, emu_library(), steps, **geom)
    assert rew > 0 and ends == int(gu.load_fixture(name)[1]["done"][:steps].sum())


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,extra,B,geom", [
    ("rware-tiny-2ag-v1", {"max_steps": 11}, 7, (4, 64)),                                            # generic kernel, ragged last chunk
    ("rware-small-4ag-v1", {"max_steps": 7, "max_inactivity_steps": 4}, 16, (0, 0)),                 # exact shape, both termination causes
    ("rware-small-10ag-v1", {"max_steps": 10}, 8, (0, 0)),                                           # per-cell agent phases
    ("rware-large-16ag-v1", {"sensor_range": 2, "max_steps": 9, "reward_type": 0}, 4, (0, 0)),        # GLOBAL rewards
    ("rware-tiny-4ag-v1", {"max_steps": 12, "reward_type": 2}, 8, (0, 0)),                           # TWO_STAGE (0.5 rewards)
])
def test_emulated_buffers_match_the_model_in_every_autoreset_mode(env_id, extra, B, geom, mode):
    check_against_model(emu_library(), env_id, extra, B, 40, mode, geom)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,B,geom", [("rware-small-4ag-v1", 16, (0, 0)), ("rware-tiny-2ag-v1", 7, (4, 64))])
def test_emulated_fused_rollout_keeps_the_order_of_add_record_clear(env_id, B, geom, mode):
    """three episode ends inside ONE launch on every env: step t's write-back and step t + 1's reset path run on different wavefronts"""
    check_rollout(emu_library(), env_id, {"max_steps": 9}, B, mode, geom)


@pytest.mark.timeout(1500)
def test_emulated_masked_reset_state_writes_and_snapshots():
    lib, B, N = emu_library(), 16, 4
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1", max_steps=9, reward_type=0)
    env = rware_amd.WarehouseVecEnv(B, library=lib, episode_stats=True, **kw)
    model = EpisodeModel(B, N, "next_step")
    env.reset(seed=4)
    acts = np.random.default_rng(6).choice(5, size=(40, B, N), p=P_ACT).astype(np.int32)

    def run(t0, t1, o=True):   # (the model follows the env's own rewards / flags here: those are the lockstep tests' business)
        for t in range(t0, t1):
            _, rew, term, _, _ = env.step(acts[t])
            if o is not None:
                model.step(rew, term)

    run(0, 5)
    # set_state seeds all five (rw_write) ...
    seed = {"ep_return": np.arange(B * N, dtype=np.float32).reshape(B, N) * 0.5, "ep_length": np.arange(B, dtype=np.int32) + 100,
            "ep_last_return": np.full((B, N), 2.5, np.float32), "ep_last_length": np.full(B, 7, np.int32), "ep_count": np.full(B, 40, np.int32)}
    env.set_state(refresh_obs=False, **seed)
    for k, n in env.EPISODE_STATS.items():
        model.v[k][...] = seed[n]
    same_buffers(env.episode_stats(), model, "seeded")
    assert all(np.array_equal(env.get_state()[n], seed[n]) for n in seed)
    run(5, 7)
    same_buffers(env.episode_stats(), model, "stepping on from the seeded values")
    # ... a masked reset mid-episode clears the running values of the masked envs only; last_* and count stay
    mask = np.arange(B) % 3 == 0
    env.reset(mask=mask)
    model.reset(mask)
    same_buffers(env.episode_stats(), model, "masked reset")
    run(7, 12)             # (through the episode end of the unmasked envs at step 9)
    same_buffers(env.episode_stats(), model, "after the masked reset")
    # snapshot, step, restore, step: identical buffers
    snap = env.snapshot()
    before = {k: v.copy() for k, v in env.episode_stats().items()}
    run(12, 24, o=None)
    later = env.episode_stats()
    assert later["count"].sum() > before["count"].sum()
    env.restore(snap)
    assert all(np.array_equal(env.episode_stats()[k], before[k]) for k in EPISODE_BUFFERS)
    run(12, 24, o=None)
    assert all(np.array_equal(env.episode_stats()[k], later[k]) for k in EPISODE_BUFFERS)
    env.free_snapshot(snap)
    env.reset(seed=4)      # reset(): running values 0, the records stay
    after = env.episode_stats()
    assert not after["return"].any() and not after["length"].any()
    assert all(np.array_equal(after[k], later[k]) for k in ("last_return", "last_length", "count"))
    env.close()


@pytest.mark.timeout(1500)
def test_emulated_sharded_env_gathers_its_buffers_in_env_order():
    B = 24
    env, orc, kw = make_pair(emu_library(), "rware-tiny-2ag-v1", {"max_steps": 9}, B, "next_step", devices=[0, 0, 0])
    assert len(env.engines) == 3
    model = EpisodeModel(B, 2, "next_step")
    rng = np.random.default_rng(9)
    env.reset(seed=3)
    orc.reset(seed=3)
    for t in range(25):
        a = rng.choice(5, size=(B, 2), p=P_ACT).astype(np.int32)
        env.step(a)
        model.step(*orc.step_autoreset(a, "next_step")[1:])
    got = env.episode_stats()
    assert got["return"].shape == (B, 2) and got["count"].shape == (B,)
    same_buffers(got, model, "sharded")
    assert model.v["count"].min() >= 2
    env.close()


@pytest.mark.timeout(1500)
def test_emulated_off_switch_and_info_bits():
    lib, B = emu_library(), 16
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    kw["max_steps"] = 6
    off = rware_amd.WarehouseVecEnv(B, library=lib, **kw)
    assert off.engines[0].episodes is False
    with pytest.raises(RuntimeError, match="episode_stats=True"):
        off.episode_stats()
    for name in off.EPISODE_STATS.values():
        with pytest.raises(rware_amd._capi.EngineError):   # the buffers are empty: zero bytes, reading B values from them is refused
            off.engines[0].read(name)
    on = rware_amd.WarehouseVecEnv(B, library=lib, episode_stats=True, **kw)
    a, b = off.engines[0].info, on.engines[0].info
    assert (a.envs_per_workgroup, a.build_kind, a.n_workgroups) == (b.envs_per_workgroup, b.build_kind, b.n_workgroups)
    assert b.lds_bytes > a.lds_bytes and b.engine_bytes_per_env_step == a.engine_bytes_per_env_step + 2 * (4 * 4 + 4)
    o0, i0 = off.reset(seed=8)
    o1, i1 = on.reset(seed=8)
    assert np.array_equal(o0, o1) and i0 == {} and i1 == {}
    acts = np.random.default_rng(2).choice(5, size=(20, B, 4), p=P_ACT).astype(np.int32)
    for t in range(20):   # the statistics change nothing else (episodes end and autoreset on the way: max_steps 6)
        x, y = off.step(acts[t]), on.step(acts[t])
        assert all(np.array_equal(p, q) for p, q in zip(x[:4], y[:4])), t
        assert x[4] == {}
        if y[2].any():    # Gymnasium's RecordEpisodeStatistics convention, on the steps that finish an episode
            assert set(y[4]) == {"episode", "_episode"} and set(y[4]["episode"]) == {"r", "l"}
            r, l, m = y[4]["episode"]["r"], y[4]["episode"]["l"], y[4]["_episode"]
            assert (r.shape, r.dtype, l.shape, l.dtype, m.shape, m.dtype) == ((B, 4), np.float32, (B,), np.int32, (B,), np.bool_)
            assert np.array_equal(m, y[2]) and (l[m] == 6).all() and not l[~m].any() and not r[~m].any()
            assert np.array_equal(r[m], on.episode_stats()["last_return"][m])
        else:
            assert y[4] == {}
    s0, s1 = off.get_state(), on.get_state()
    assert all(np.array_equal(v, s1[k]) for k, v in s0.items()) and set(s1) - set(s0) == set(on.EPISODE_STATS.values())
    off.close()
    on.close()
    for stats, episodes, want in [(False, False, 0), (True, False, 1), (False, True, 2), (True, True, 3)]:
        env = rware_amd.WarehouseVecEnv(B, library=lib, stats=stats, episode_stats=episodes, **kw)
        assert env.engines[0].info.stats == want and (env.engines[0].stats, env.engines[0].episodes) == (stats, episodes)
        env.close()


@pytest.mark.timeout(1500)
def test_emulated_statistics_combine_with_counters_and_packed_rows():
    """RW_STATS_ON | RW_OBS_PACKED | RW_EPISODES_ON on one engine: the event counters, the packed rows and the five buffers all hold"""
    B = 8
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1", max_steps=8)
    env = rware_amd.WarehouseVecEnv(B, library=emu_library(), episode_stats=True, stats=True, obs_format="packed", **kw)
    orc = OracleVecEnv(B, **kw)
    model = EpisodeModel(B, 2, "next_step")
    rng = np.random.default_rng(3)
    assert np.array_equal(env.unpack_obs(env.reset(seed=2)[0]), orc.reset(seed=2))
    for t in range(20):
        a = rng.choice(5, size=(B, 2), p=P_ACT).astype(np.int32)
        obs = env.step(a)[0]
        o2, r2, d2 = orc.step_autoreset(a, "next_step")
        model.step(r2, d2)
        assert np.array_equal(env.unpack_obs(obs), o2), t
        same_buffers(env.episode_stats(), model, t)
    c = env.event_counters()
    assert np.array_equal(c["failed_moves"], orc.stat_failed_moves) and np.array_equal(c["deliveries"], orc.stat_deliveries)
    assert model.v["count"].min() >= 2
    env.close()


@pytest.mark.timeout(1500)
def test_emulated_pipelined_request_falls_back_to_the_classic_kernel():
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    env = rware_amd.WarehouseVecEnv(32, library=emu_library(), episode_stats=True, pipe=True, **kw)
    assert env.engines[0].info.pipe_workgroups == 0 and "RW_EPISODES_ON" in env.engines[0].jit_log()
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------
# GPU suite: the gfx950 library, through the C-ABI
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", gu.fixture_names())
def test_engine_and_model_agree_on_the_references_traces(name):
    """every golden trace in full on the device: the recorded rewards / done flags through the model, the actions through the engine"""
    meta, z = gu.load_fixture(name)
    ends, _ = replay_golden(name, None)
    assert ends == int(z["done"].sum())


@pytest.mark.gpu
def test_some_golden_trace_ends_an_episode():
    assert sum(int(gu.load_fixture(n)[1]["done"].sum()) for n in gu.fixture_names()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,extra,B,jit", [
    ("rware-small-4ag-v1", {"max_steps": 9, "max_inactivity_steps": 6}, 64, True),   # run-time compiled exact-shape build
    ("rware-tiny-2ag-v1", {"max_steps": 8}, 7, None),                               # generic kernel, ragged last chunk
    ("rware-small-10ag-v1", {"max_steps": 10}, 32, True),                           # per-cell agent phases
    ("rware-large-16ag-v1", {"sensor_range": 2, "max_steps": 11, "reward_type": 0}, 16, True),
    ("rware-small-19ag-v1", {"max_steps": 12}, 8, None),
])
def test_buffers_match_the_model_in_every_autoreset_mode(env_id, extra, B, jit, mode):
    check_against_model(None, env_id, extra, B, 40, mode, jit=jit)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,extra,B", [("rware-small-4ag-v1", {}, 64), ("rware-large-16ag-v1", {"sensor_range": 2}, 16)])
def test_fused_rollout_keeps_the_order_of_add_record_clear(env_id, extra, B, mode):
    check_rollout(None, env_id, dict(extra, max_steps=9), B, mode, jit=True)


@pytest.mark.gpu
def test_an_engine_with_episode_statistics_gets_a_kernel_that_keeps_them(tmp_path, monkeypatch):
    """rw_create's choice, as for the event counters: the generic kernel below 4096 envs, a run-time compiled exact-shape build from there on
    (rw_jit_log says why); without the flag the ahead-of-time build and no buffers"""
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    plain = rware_amd.WarehouseVecEnv(4096, **kw)
    i = plain.engines[0].info
    assert (i.stats, i.jit, i.build_kind) == (0, 0, 1) and plain.engines[0].jit_log() == ""
    big = rware_amd.WarehouseVecEnv(4096, episode_stats=True, **kw)
    j = big.engines[0].info
    assert (j.stats, j.jit, j.build_kind, j.specialised) == (2, 1, 1, 1), big.engines[0].jit_log()
    assert "episode statistics" in big.engines[0].jit_log()
    small = rware_amd.WarehouseVecEnv(64, episode_stats=True, **kw)
    k = small.engines[0].info
    assert (k.stats, k.jit, k.build_kind) == (2, 0, 0)
    for e in (plain, big, small):
        e.close()


@pytest.mark.gpu
def test_statistics_are_zero_copy_tensors_current_after_a_captured_loop():
    """output="torch": the five tensors alias the engine's buffers and are current after capture_loop(...).replay() without a copy — the
    form a closed loop that never shows the host a step reads"""
    import torch

    B, N, K = 64, 4, 12
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1", max_steps=5)
    env = rware_amd.WarehouseVecEnv(B, output="torch", episode_stats=True, **kw)
    orc = OracleVecEnv(B, **kw)
    model = EpisodeModel(B, N, "next_step")
    env.reset(seed=31)
    orc.reset(seed=31)
    st = env.episode_stats()
    for k, n in env.EPISODE_STATS.items():
        assert st[k].is_cuda and st[k].data_ptr() == env.engines[0].device_array(n).ptr
    assert st["return"].dtype == torch.float32 and st["return"].shape == (B, N) and st["count"].dtype == torch.int32
    tape = np.random.default_rng(4).choice(5, size=(K, B, N), p=P_ACT).astype(np.int32)
    dev_tape = torch.from_numpy(tape).cuda()
    cursor = torch.zeros((), dtype=torch.long, device="cuda")

    def policy(obs, rewards, terminated):   # a capturable open-loop policy: row `cursor` of the tape, then cursor += 1
        a = dev_tape.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return a

    loop = env.capture_loop(policy, steps=K, warmup=0)
    cursor.zero_()
    loop.replay()
    torch.cuda.synchronize()
    for t in range(K):
        model.step(*orc.step_autoreset(tape[t], "next_step")[1:])
    same_buffers({k: v.cpu().numpy() for k, v in st.items()}, model, "after the replay")   # the SAME tensors, now current
    assert model.v["count"].min() >= 2
    _, _, _, _, info = env.step(dev_tape[0])
    assert info == {}   # torch output: no host synchronisation, no keys
    env.close()
