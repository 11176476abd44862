"""Time-limit ends reported as truncation (rw_stream_flags RW_TIME_LIMIT_TRUNCATES; WarehouseVecEnv(time_limit_truncates=True)).

The reference reports every end of an episode as `terminated` (rware/warehouse.py:935-942).  With the flag the engine reports the step
limit as `truncated` and only the inactivity limit as `terminated`; `terminated | truncated` stays the reference's `done`.  The expected
split comes from the ORACLE, not from the engine: OracleVecEnv.step is wrapped (tap_split), and when it returns — before step_autoreset
resets anything — the two rules of the contract (include/rware_hip.h at the flag) are evaluated on the oracle's own counters for the envs
it stepped and asserted to add up to the oracle's `done`.  The env is driven through lockstep.lockstep behind a thin adapter that hands the
harness `terminated | truncated` as `terminated` (the invariant, compared with the oracle's `done` on every step) and keeps the raw pair.
  - CPU suite: the product sources on host threads (tests/emu);
  - GPU suite (-m gpu): the gfx950 library — the generic kernel and run-time compiled exact-shape builds, a captured loop with torch output.
"""
import numpy as np
import pytest

import golden_util as gu
import lockstep
from device_backends import emu_library
from models import EpisodeModel, same_buffers
from rware_oracle import OracleVecEnv

import rware_amd

MODES = ["next_step", "same_step", "disabled"]
P_ACT = [.05, .7, .1, .1, .05]
# (env id, B, (envs, threads) per workgroup, generic?): the generic kernel with a ragged last chunk; the exact-shape builds of the register
# agent phase (2 agents) and of the per-cell LDS phase (9 agents)
EMU_BUILDS = [("rware-tiny-2ag-v1", (4, 64), True), ("rware-tiny-2ag-v1", (0, 0), False), ("rware-tiny-9ag-v1", (0, 0), False)]


def tap_split(orc, kw):
    """Wraps orc.step: orc.split = (by_inactivity, by_steps) of the latest step, from the oracle's counters right behind the step (nothing
    is reset yet); envs the call did not step (a NEXT_STEP reset step) expect 0 / 0.  The two rules must add up to the oracle's `done`."""
    inner, ms, mi = orc.step, int(kw.get("max_steps") or 0), int(kw.get("max_inactivity_steps") or 0)

    def step(actions, mask=None):
        rew, done = inner(actions, mask)
        stepped = np.ones(orc.B, bool) if mask is None else np.asarray(mask, bool)
        by_steps = stepped & (ms != 0) & (orc.steps >= ms)
        by_inact = stepped & (mi != 0) & (orc.inactive >= mi)
        assert np.array_equal(by_steps | by_inact, done.astype(bool)), "the model of the split does not add up to the oracle's done"
        orc.split = (by_inact, by_steps)
        return rew, done

    orc.step = step
    return orc


class Adapter:
    """What lockstep.lockstep steps: `terminated | truncated` as `terminated`, zeros as `truncated`; `raw` keeps the pair."""

    def __init__(self, env):
        self.env, self.raw = env, None

    def __getattr__(self, k):
        return getattr(self.env, k)

    def step(self, a):
        obs, rew, term, trunc, info = self.env.step(a)
        assert term.dtype == np.bool_ and trunc.dtype == np.bool_ and term.shape == trunc.shape == (self.env.num_envs,)
        self.raw = (term.copy(), trunc.copy())
        return obs, rew, term | trunc, np.zeros_like(trunc), info


def same_split(raw, orc, what):
    for got, want, name in zip(raw, orc.split, ("terminated", "truncated")):
        assert np.array_equal(np.asarray(got, bool), want), (name, what, np.argwhere(np.asarray(got, bool) != want)[:5].tolist())


def make_pair(lib, env_id, extra, B, mode, geom=(0, 0), jit=None, generic=None, **env_kw):
    kw = lockstep.oracle_kwargs(env_id, **extra)
    env = rware_amd.WarehouseVecEnv(B, autoreset_mode=mode, library=lib, time_limit_truncates=True, envs_per_workgroup=geom[0],
                                    threads_per_workgroup=geom[1], jit=jit, **env_kw, **kw)
    info = env.engines[0].info
    assert info.stats & 8 and env.engines[0].time_limit_truncates
    assert not jit or info.jit in (1, 2), env.engines[0].jit_log()
    assert generic is None or (info.build_kind == 0) == generic, (info.build_kind, env.engines[0].jit_log())
    return env, tap_split(OracleVecEnv(B, **kw), kw), kw


def check_constructed(lib, env_id, mode, geom=(0, 0), jit=None, generic=None, B=32):
    """the four cases in neighbouring envs of one workgroup: step limit only, inactivity only, both, neither — one all-NOOP step"""
    env, orc, kw = make_pair(lib, env_id, {"max_steps": 12, "max_inactivity_steps": 5}, B, mode, geom, jit, generic)
    N = kw["n_agents"]
    env.reset(seed=3)
    orc.reset(seed=3)
    steps = np.array([11, 0, 11, 3], np.int32)[np.arange(B) % 4]
    inact = np.array([0, 4, 4, 1], np.int32)[np.arange(B) % 4]
    env.set_state(steps=steps, inactive=inact)
    orc.set_state(steps=steps, inactive=inact)
    noop = np.zeros((B, N), np.int32)
    want_term, want_trunc = np.isin(np.arange(B) % 4, (1, 2)), np.isin(np.arange(B) % 4, (0, 2))   # (case 3: neither)
    for t in range(3):   # the constructed step; then what each mode does with the finished envs (reset step / fresh episode / stepped on)
        obs, rew, term, trunc, info = env.step(noop)
        o2, r2, d2 = orc.step_autoreset(noop, mode)
        lockstep.same_obs(obs, o2, "obs", t)
        assert np.array_equal(term | trunc, d2.astype(bool)), (mode, t)
        same_split((term, trunc), orc, (mode, t))
        if t == 0:
            assert np.array_equal(term, want_term) and np.array_equal(trunc, want_trunc) and (term & trunc).any()
        if mode == "same_step":
            assert ("final_obs" in info) == bool(d2.any())
            if d2.any():
                assert np.array_equal(info["_final_obs"], term | trunc)
    lockstep.same_state(env.get_state(), orc.get_state(), "end")
    env.close()


def check_lockstep(lib, env_id, extra, B, T, mode, geom=(0, 0), jit=None, generic=None, seed=17):
    env, orc, kw = make_pair(lib, env_id, extra, B, mode, geom, jit, generic)
    ad = Adapter(env)
    rng = np.random.default_rng(seed)
    ends, seen = np.zeros(B, int), {"term": 0, "trunc": 0, "first_inact": 0}

    def split(t, obs, rew, done, info):
        same_split(ad.raw, orc, (mode, t))
        term, trunc = ad.raw
        assert np.array_equal(term | trunc, done)
        ends[...] += done
        seen["term"] += int(term.sum())
        seen["trunc"] += int(trunc.sum())
        seen["first_inact"] += int((term & ~trunc).sum())

    lockstep.lockstep(ad, orc, lambda t: rng.choice(5, size=(B, kw["n_agents"]), p=P_ACT).astype(np.int32), mode, seed=seed, steps=T,
                      on_step=split)
    assert ends.max() >= 2, "the run finished fewer than two episodes on every env: it proves nothing"
    env.close()
    return seen


def check_rollout(lib, env_id, B, mode, geom=(0, 0), jit=None, generic=None, T=30):
    """one fused launch of T steps == T single steps == the model, on the truncated tape too; three single steps carry on"""
    extra = {"max_steps": 7}
    env, orc, kw = make_pair(lib, env_id, extra, B, mode, geom, jit, generic)
    single, _, _ = make_pair(lib, env_id, extra, B, mode, geom, jit, generic)
    N = kw["n_agents"]
    for e in (env, orc, single):
        e.reset(seed=5)
    acts = np.random.default_rng(1).choice(5, size=(T + 3, B, N), p=P_ACT).astype(np.int32)
    out = env.rollout(acts[:T], want_obs=False)
    assert len(out) == 4
    _, rew, term, trunc = out
    assert term.dtype == np.bool_ and trunc.dtype == np.bool_ and trunc.shape == (T, B)
    ends = np.zeros(B, int)
    for t in range(T):
        _, r2, d2 = orc.step_autoreset(acts[t], mode)
        _, r1, t1, u1, _ = single.step(acts[t])
        assert np.array_equal(rew[t], r2) and np.array_equal(term[t] | trunc[t], d2.astype(bool)), t
        same_split((term[t], trunc[t]), orc, (mode, "tape", t))
        assert np.array_equal(term[t], t1) and np.array_equal(trunc[t], u1), t
        ends += d2.astype(bool)
    # max_steps 7: an end every 7 steps, in NEXT_STEP every 8 (the reset step) — T = 30 holds four of the former, three of the latter;
    # DISABLED: every step from the seventh on
    assert ends.min() >= (3 if mode == "next_step" else 4) and not term.any() and trunc.any()
    for t in range(T, T + 3):
        _, _, term1, trunc1, _ = env.step(acts[t])
        d2 = orc.step_autoreset(acts[t], mode)[2]
        assert np.array_equal(term1 | trunc1, d2.astype(bool))
        same_split((term1, trunc1), orc, (mode, t))
    # a fused launch without tapes: its last step's flags land in the buffers, as for `terminated`
    # (T + 3 = 33 steps so far; the next end: step 39 in NEXT_STEP — ends at 7, 15, 23, 31 —, 35 and 42 in SAME_STEP, every step in DISABLED)
    eng, more = env.engines[0], np.ascontiguousarray(acts[:{"next_step": 6, "same_step": 9, "disabled": 2}[mode]])
    d_a = eng.scratch("tl_actions", more.nbytes)
    eng._check(eng.lib.rw_copy_to_device(eng._h, d_a, more.ctypes.data, more.nbytes))
    eng.step_many_device(d_a.value, len(more))
    for a in more:
        orc.step_autoreset(a, mode)
    same_split((eng.read("terminated"), eng.read("truncated")), orc, (mode, "no tape"))
    assert orc.split[1].all()   # (that last step truncates every env)
    lockstep.same_state(env.get_state(), orc.get_state(), "end")
    env.close()
    single.close()


def check_rollout_without_the_flag(lib, B=8, T=5):
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1", max_steps=3)
    env = rware_amd.WarehouseVecEnv(B, library=lib, **kw)
    env.reset(seed=1)
    acts = np.zeros((T, B, 2), np.int32)
    out = env.rollout(acts, want_obs=False)
    assert len(out) == 3 and out[2].any()
    eng = env.engines[0]
    d_a, d_u = eng.scratch("tl_actions", acts.nbytes), eng.scratch("tl_truncated", T * B)
    fill = np.full(T * B, 0xff, np.uint8)
    eng._check(eng.lib.rw_copy_to_device(eng._h, d_a, acts.ctypes.data, acts.nbytes))
    eng._check(eng.lib.rw_copy_to_device(eng._h, d_u, fill.ctypes.data, fill.nbytes))
    eng.step_many_device(d_a.value, T, truncated_tape=d_u.value)
    eng.read_scratch("tl_truncated", fill)
    assert not fill.any()   # zero-filled: nothing truncates without the flag
    env.close()


class GoldenBackend:
    """golden_util.replay's backend: the env behind the adapter's rule, an oracle with the split beside it"""

    def __init__(self, meta, lib, **env_kw):
        kw = gu.ctor_kwargs(meta)
        self.env = rware_amd.WarehouseVecEnv(meta["E"], library=lib, time_limit_truncates=True, **env_kw, **kw)
        self.orc = tap_split(OracleVecEnv(meta["E"], **kw), kw)
        self.seen = {"term": 0, "trunc": 0}

    def reset(self, seed=None):
        self.orc.reset(seed=seed)
        o = self.env.reset(seed=seed)[0]
        return (o["image"], o["features"]) if isinstance(o, dict) else o

    def step_autoreset(self, actions, mode):
        obs, rew, term, trunc, _ = self.env.step(actions)
        self.orc.step_autoreset(actions, mode)
        same_split((term, trunc), self.orc, "golden")
        self.seen["term"] += int(term.sum())
        self.seen["trunc"] += int(trunc.sum())
        return ((obs["image"], obs["features"]) if isinstance(obs, dict) else obs), rew, term | trunc

    def get_state(self):
        return self.env.get_state()


def replay_golden(name, lib, **env_kw):
    meta, z = gu.load_fixture(name)
    b = GoldenBackend(meta, lib, **env_kw)
    gu.replay(b, meta, z)   # observations, rewards and state equal the recorded ones; terminated | truncated the recorded `done`
    b.env.close()
    return b.seen


# ------------------------------------------------------------------------------------------------------------------------------
# CPU suite: the product sources on host threads
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(1500)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,geom,generic", EMU_BUILDS)
def test_emulated_four_cases_in_one_workgroup(env_id, geom, generic, mode):
    check_constructed(emu_library(), env_id, mode, geom, generic=generic)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,geom,generic", EMU_BUILDS)
def test_emulated_lockstep_every_end_is_a_truncation(env_id, geom, generic, mode):
    seen = check_lockstep(emu_library(), env_id, {"max_steps": 6}, 12 if generic else 16, 40, mode, geom, generic=generic)
    assert seen["term"] == 0 and seen["trunc"] > 0


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,geom,generic", EMU_BUILDS)
def test_emulated_lockstep_inactivity_ends_come_first(env_id, geom, generic, mode):
    seen = check_lockstep(emu_library(), env_id, {"max_steps": 9, "max_inactivity_steps": 4}, 12 if generic else 16, 40, mode, geom, generic=generic)
    assert seen["first_inact"] > 0


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,geom,generic", EMU_BUILDS[:2])
def test_emulated_fused_rollout_tapes_the_truncated_flags(env_id, geom, generic, mode):
    check_rollout(emu_library(), env_id, 7 if generic else 16, mode, geom, generic=generic)


@pytest.mark.timeout(1500)
def test_emulated_rollout_without_the_flag_keeps_three_elements_and_zero_fills_a_tape():
    check_rollout_without_the_flag(emu_library())


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("name,geom,kinds", [
    ("img-square-all7-msg1", {}, ("term", "trunc")),     # IMAGE, messages, max_steps 100 / max_inactivity 40: both kinds of end
    ("medium-2ag-easy", {"envs_per_workgroup": 4, "threads_per_workgroup": 64}, ("trunc",)),   # max_steps 150, no inactivity limit
])
def test_emulated_engine_replays_the_references_traces_with_the_flag(name, geom, kinds):
    seen = replay_golden(name, emu_library(), **geom)
    assert all(seen[k] > 0 for k in kinds) and (seen["term"] == 0 or "term" in kinds)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_truncating_step_records_the_episode(mode):
    """episode_stats=True: the record follows `done`, not `terminated` — EpisodeModel fed with the oracle's done; numpy step()'s info keys"""
    B = 16
    env, orc, kw = make_pair(emu_library(), "rware-small-4ag-v1", {"max_steps": 7, "max_inactivity_steps": 5}, B, mode, episode_stats=True)
    model = EpisodeModel(B, 4, mode)
    rng = np.random.default_rng(2)
    env.reset(seed=9)
    orc.reset(seed=9)
    for t in range(30):
        a = rng.choice(5, size=(B, 4), p=P_ACT).astype(np.int32)
        _, _, term, trunc, info = env.step(a)
        _, r2, d2 = orc.step_autoreset(a, mode)
        model.step(r2, d2)
        same_split((term, trunc), orc, (mode, t))
        same_buffers(env.episode_stats(), model, (mode, t))
        if d2.any():
            assert np.array_equal(info["_episode"], d2.astype(bool))
            assert np.array_equal(info["episode"]["l"][info["_episode"]], model.v["last_length"][info["_episode"]])
        else:
            assert "episode" not in info
    assert model.v["count"].min() >= 2
    env.close()


@pytest.mark.timeout(1500)
def test_emulated_resets_snapshots_and_numpy_step():
    B, N = 16, 4
    env, orc, kw = make_pair(emu_library(), "rware-small-4ag-v1", {"max_steps": 6}, B, "disabled")
    acts = np.random.default_rng(6).choice(5, size=(20, B, N), p=P_ACT).astype(np.int32)
    env.reset(seed=4)
    for t in range(6):
        _, _, term, trunc, info = env.step(acts[t])
    assert trunc.dtype == np.bool_ and trunc.all() and not term.any() and info == {}
    assert env.engines[0].read("truncated").all()
    # a masked reset clears `truncated` of the masked envs only
    mask = np.arange(B) % 3 == 0
    env.reset(mask=mask)
    assert np.array_equal(env.engines[0].read("truncated").astype(bool), ~mask)
    assert not env.engines[0].read("terminated").any()
    # snapshot, step, restore, step: the same flags again
    snap = env.snapshot()
    first = [env.step(acts[t])[2:4] for t in range(6, 14)]
    env.restore(snap)
    again = [env.step(acts[t])[2:4] for t in range(6, 14)]
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(first, again))
    assert any(a[1].any() and not a[1].all() for a in first)   # (the envs reset above end later than the others)
    env.free_snapshot(snap)
    with pytest.raises(rware_amd._capi.EngineError, match="read-only"):   # still no input
        env.engines[0].write("truncated", np.zeros(B, np.uint8))
    env.close()


@pytest.mark.timeout(1500)
def test_emulated_sharded_env_concatenates_the_flags():
    B = 24
    env, orc, kw = make_pair(emu_library(), "rware-tiny-2ag-v1", {"max_steps": 9, "max_inactivity_steps": 6}, B, "next_step", devices=[0, 0, 0])
    assert len(env.engines) == 3 and all(e.time_limit_truncates for e in env.engines)
    seen = {"term": 0, "trunc": 0}
    rng = np.random.default_rng(9)
    env.reset(seed=3)
    orc.reset(seed=3)
    steps = (np.arange(B) % 7).astype(np.int32)   # staggered: which rule ends the first episode depends on the env, within every shard
    env.set_state(steps=steps)
    orc.set_state(steps=steps)
    for t in range(25):
        a = rng.choice(5, size=(B, 2), p=P_ACT).astype(np.int32)
        _, _, term, trunc, _ = env.step(a)
        orc.step_autoreset(a, "next_step")
        same_split((term, trunc), orc, t)
        seen["term"] += int(term.sum())
        seen["trunc"] += int(trunc.sum())
    assert seen["term"] > 0 and seen["trunc"] > 0
    out = env.rollout(rng.choice(5, size=(4, B, 2), p=P_ACT).astype(np.int32), want_obs=False)
    assert len(out) == 4 and out[3].shape == (4, B)
    env.close()


@pytest.mark.timeout(1500)
def test_emulated_off_switch_and_table():
    lib, B = emu_library(), 16
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1", max_steps=6)
    off = rware_amd.WarehouseVecEnv(B, library=lib, **kw)
    on = rware_amd.WarehouseVecEnv(B, library=lib, time_limit_truncates=True, **kw)
    orc = OracleVecEnv(B, **kw)
    a, b = off.engines[0].info, on.engines[0].info
    assert a.stats == 0 and b.stats == 8 and off.engines[0].time_limit_truncates is False
    assert (a.envs_per_workgroup, a.n_workgroups, a.lds_bytes) == (b.envs_per_workgroup, b.n_workgroups, b.lds_bytes)
    assert b.engine_bytes_per_env_step == a.engine_bytes_per_env_step + 1
    # (this library's exact-shape builds carry the code: the same kernel as without the flag; the gfx950 library's choice is a GPU test)
    assert b.build_kind == a.build_kind and b.jit == 0
    assert len(rware_amd._capi.BUFFERS) == 29
    for e in (off, on, orc):
        e.reset(seed=8)
    acts = np.random.default_rng(2).choice(5, size=(20, B, 4), p=P_ACT).astype(np.int32)
    for t in range(20):
        x, y = off.step(acts[t]), on.step(acts[t])
        d2 = orc.step_autoreset(acts[t], "next_step")[2].astype(bool)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[4] == {} and y[4] == {}
        assert not x[3].any() and np.array_equal(x[2], d2)             # no flag: the reference's flags
        assert np.array_equal(y[2] | y[3], d2) and not y[2].any()      # flag: max_steps only, every end a truncation
    s0, s1 = off.get_state(), on.get_state()
    assert set(s0) == set(s1) and all(np.array_equal(v, s1[k]) for k, v in s0.items())
    for env in (off, on):
        with pytest.raises(rware_amd._capi.EngineError, match="read-only"):
            env.engines[0].write("truncated", np.zeros(B, np.uint8))
    off.close()
    on.close()
    env = rware_amd.WarehouseVecEnv(B, library=lib, time_limit_truncates=True, stats=True, episode_stats=True, action_mask=True, **kw)
    assert env.engines[0].info.stats == 15
    env.close()
    env = rware_amd.WarehouseVecEnv(32, library=lib, time_limit_truncates=True, pipe=True, **kw)
    assert env.engines[0].info.pipe_workgroups == 0 and "RW_TIME_LIMIT_TRUNCATES" in env.engines[0].jit_log()
    env.close()
    assert rware_amd.make_vec("rware-tiny-2ag-v1", 4, library=lib, time_limit_truncates=True).engines[0].time_limit_truncates


# ------------------------------------------------------------------------------------------------------------------------------
# GPU suite: the gfx950 library, through the C-ABI
# ------------------------------------------------------------------------------------------------------------------------------
GPU_BUILDS = [("rware-tiny-2ag-v1", None, True), ("rware-tiny-2ag-v1", True, False), ("rware-tiny-9ag-v1", True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,jit,generic", GPU_BUILDS)
def test_four_cases_in_one_workgroup(env_id, jit, generic, mode):
    check_constructed(None, env_id, mode, jit=jit, generic=generic)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,jit,generic", GPU_BUILDS)
def test_lockstep_every_end_is_a_truncation(env_id, jit, generic, mode):
    seen = check_lockstep(None, env_id, {"max_steps": 6}, 32, 40, mode, jit=jit, generic=generic)
    assert seen["term"] == 0 and seen["trunc"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id,jit,generic", GPU_BUILDS[:2])
def test_fused_rollout_tapes_the_truncated_flags(env_id, jit, generic, mode):
    check_rollout(None, env_id, 32, mode, jit=jit, generic=generic)


@pytest.mark.gpu
def test_an_engine_with_the_flag_gets_a_kernel_that_carries_the_code():
    """rw_create's choice, as for the other RW_STATS_BUILD outputs: below 4096 envs the generic kernel, and rw_jit_log names the flag"""
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    plain = rware_amd.WarehouseVecEnv(64, **kw)
    small = rware_amd.WarehouseVecEnv(64, time_limit_truncates=True, **kw)
    i, k = plain.engines[0].info, small.engines[0].info
    assert (i.stats, i.jit, i.build_kind) == (0, 0, 1) and plain.engines[0].jit_log() == ""
    assert (k.stats, k.jit, k.build_kind) == (8, 0, 0) and "time-limit truncation" in small.engines[0].jit_log()
    plain.close()
    small.close()


@pytest.mark.gpu
def test_rollout_without_the_flag_keeps_three_elements_and_zero_fills_a_tape():
    check_rollout_without_the_flag(None)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kinds", [("img-square-all7-msg1", ("term", "trunc")), ("medium-2ag-easy", ("trunc",))])
def test_engine_replays_the_references_traces_with_the_flag(name, kinds):
    seen = replay_golden(name, None)
    assert all(seen[k] > 0 for k in kinds) and (seen["term"] == 0 or "term" in kinds)


@pytest.mark.gpu
def test_truncated_is_a_live_zero_copy_tensor_under_a_captured_loop():
    """output="torch": device_tensor("truncated") is the same storage every round and holds the model's flags after each replay"""
    import torch

    B, N, K = 64, 4, 12
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1", max_steps=5)
    env = rware_amd.WarehouseVecEnv(B, output="torch", time_limit_truncates=True, **kw)
    orc = tap_split(OracleVecEnv(B, **kw), kw)
    env.reset(seed=31)
    orc.reset(seed=31)
    trunc, term = env.device_tensor("truncated"), env.device_tensor("terminated")
    ptr = env.engines[0].device_array("truncated").ptr
    assert trunc.is_cuda and trunc.data_ptr() == ptr and trunc.dtype == torch.uint8 and trunc.shape == (B,)
    tape = np.random.default_rng(4).choice(5, size=(2 * K, B, N), p=P_ACT).astype(np.int32)
    dev_tape = torch.from_numpy(tape).cuda()
    cursor = torch.zeros((), dtype=torch.long, device="cuda")

    acc = torch.zeros(B, dtype=torch.int32, device="cuda")

    def policy(obs, rewards, terminated):   # a capturable open-loop policy: row `cursor` of the tape, then cursor += 1 ...
        acc.add_(trunc)                      # ... which reads the truncated tensor on every round: the previous step's flags
        a = dev_tape.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return a

    loop = env.capture_loop(policy, steps=K, warmup=0)
    cursor.zero_()
    acc.zero_()
    want = np.zeros(B, np.int32)
    for r in range(2):
        loop.replay()
        torch.cuda.synchronize()
        for t in range(r * K, (r + 1) * K):
            orc.step_autoreset(tape[t], "next_step")
            want += orc.split[1] if t < 2 * K - 1 else 0   # (no round reads the last step's flags)
        assert env.device_tensor("truncated").data_ptr() == ptr
        same_split((term.cpu().numpy(), trunc.cpu().numpy()), orc, ("replay", r))   # the SAME tensors, now current
    # max_steps 5, NEXT_STEP: an end at steps 5, 11, 17 and 23, a reset step behind each (so both replays end on 0 / 0)
    assert np.array_equal(acc.cpu().numpy(), want) and (want == 4).all() and not orc.split[1].any()
    env.close()
