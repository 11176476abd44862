"""Per-agent valid-action masks written by the step kernels (rw_stream_flags RW_ACTION_MASK_ON; WarehouseVecEnv(action_mask=True)).

The reference has no mask (its `info` is {}), so the contract — include/rware_hip.h at RW_ACTION_MASK_ON — is stated in terms of what the
reference's step() does, and checked that way:
  - `solo_probe`: an OracleVecEnv of B * N * 4 envs, set to the oracle's state, tiled; copy (e, i, a) gives agent i action a and every
    other agent NOOP and takes one step.  Strict bit a (1..4) == "(x, y, dir, carrying_shelf) of agent i changed".  The independent check.
  - `mask_model`: all six bits from a get_state() dict and the highway array in plain numpy — the contract's text.  Every lockstep run
    pins it against `solo_probe` (bits 1..4) after the reset and every 10th step, so it cannot drift from the reference's behaviour.
Lockstep runs drive env beside oracle through lockstep.lockstep (every field of the step still compared) and compare the raw byte, the
bool (B, N, 5) form (strict and permissive) and info["action_mask"] against the model after the reset and after every step.  A run must
MEET every case (a wall, a standing shelf in front of a loaded agent, an agent ahead, TOGGLE_LOAD valid and invalid both loaded and
unloaded, an env reset inside the run), counted on the oracle's state, or it fails: it would prove nothing.  DISABLED never resets by
itself, so those runs reset half of the terminated envs once, explicitly (a masked reset), and carry on.
Bit 5 (FORWARD_IF_VACATED) has its own operational check on constructed states: the occupant is given a free way out, both agents
request FORWARD, the follower moves iff bit 5.
  - CPU suite: the product sources on host threads (tests/emu), where every exact-shape build carries the code;
  - GPU suite (-m gpu): the gfx950 library — the generic kernels and run-time compiled exact-shape builds (jit="force").
"""
from collections import Counter

import numpy as np
import pytest

import lockstep
from device_backends import emu_library
from models import bits, mask_model
from rware_oracle import OracleVecEnv

import rware_amd

MODES = ["next_step", "same_step", "disabled"]
P_ACT = [.05, .5, .1, .1, .25]
MAX_STEPS, STEPS, SEED = 25, 60, 17
UP, DOWN, LEFT, RIGHT = 0, 1, 2, 3
NOOP, FORWARD, TURN_LEFT, TURN_RIGHT, TOGGLE = 0, 1, 2, 3, 4
CASES = ("wall", "standing_shelf_while_loaded", "agent_ahead", "toggle_valid_unloaded", "toggle_invalid_unloaded",
         "toggle_valid_loaded", "toggle_invalid_loaded", "reset")


def solo_probe(orc, kw):
    """bool (B, N, 4): [e, i, a - 1] — did the reference step in which agent i of env e requests a and everybody else NOOP change the
    agent's (x, y, dir, carrying_shelf)"""
    st = orc.get_state()
    B, N, M = orc.B, orc.N, orc.M
    probe = OracleVecEnv(B * N * 4, **kw)
    probe.set_state(**{k: np.repeat(v, N * 4, axis=0) for k, v in st.items()})
    a = np.zeros((B, N, 4, N, 1 + M), np.int32)
    for i in range(N):
        a[:, i, np.arange(4), i, 0] = np.arange(1, 5)
    rec = lambda: np.stack([probe.agent_x, probe.agent_y, probe.agent_dir, probe.agent_carry], -1).reshape(B, N, 4, N, 4).copy()
    before = rec()
    probe.step(a.reshape(B * N * 4, N, 1 + M))
    changed = (rec() != before).any(-1)                     # (B, N, 4, N)
    i = np.arange(N)
    return changed[:, i, :, i].transpose(1, 0, 2)           # agent i in the copies that moved agent i


def raw_bytes(env):
    return np.concatenate([eng.read("action_mask") for eng in env.engines], axis=0)


def same_mask(env, orc, what, info=None):
    """the raw byte, the bool forms and info["action_mask"] against the model of the oracle's state; returns the cases met"""
    want, met = mask_model(orc.get_state(), orc.hw)
    got = raw_bytes(env)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist(), got[got != want][:5], want[got != want][:5])
    m = env.action_mask()
    assert m.dtype == np.bool_ and m.shape == want.shape + (5,) and np.array_equal(m, bits(want)), what
    assert np.array_equal(env.action_mask(permissive=True), bits(want, True)), what
    if info is not None:
        assert np.array_equal(info["action_mask"], bits(want)) and info["action_mask"].dtype == np.bool_, what
    return met


def model_matches_probe(orc, kw, what):
    want, _ = mask_model(orc.get_state(), orc.hw)
    probe = solo_probe(orc, kw)
    assert np.array_equal(bits(want)[..., 1:], probe), (what, np.argwhere(bits(want)[..., 1:] != probe)[:5].tolist())


def make_env(lib, kw, B, mode="next_step", jit=None, **env_kw):
    env = rware_amd.WarehouseVecEnv(B, autoreset_mode=mode, library=lib, action_mask=True, jit=jit, **env_kw, **kw)
    assert not jit or env.engines[0].info.jit in (1, 2), env.engines[0].jit_log()
    assert env.engines[0].info.stats & 4
    return env


def check_lockstep(lib, env_id, extra, B, mode, jit=None, **env_kw):
    kw = lockstep.oracle_kwargs(env_id, **dict(extra, max_steps=MAX_STEPS))
    env, orc = make_env(lib, kw, B, mode, jit, **env_kw), OracleVecEnv(B, **kw)
    N, M = kw["n_agents"], kw.get("msg_bits", 0)
    rng = np.random.default_rng(SEED)
    met = Counter()

    def actions(t):
        a = rng.choice(5, size=(B, N), p=P_ACT).astype(np.int32)
        return np.concatenate([a[..., None], rng.integers(0, 2, size=(B, N, M), dtype=np.int32)], -1) if M else a

    obs, info = env.reset(seed=SEED)
    lockstep.same_obs(obs, orc.reset(seed=SEED), "reset obs", "reset")
    met.update(same_mask(env, orc, "reset", info))
    model_matches_probe(orc, kw, "reset")

    def on_step(t, obs, rew, term, info):
        met.update(same_mask(env, orc, (mode, t), info))
        if t % 10 == 9:
            model_matches_probe(orc, kw, (mode, t))
        term = np.asarray(term, bool)
        if mode == "same_step" or (mode == "next_step" and t + 1 < STEPS):
            met["reset"] += int(term.sum())                 # reset in this step / by the next one
        if mode == "disabled" and t == 30:                  # (every env terminated at step 25 and stays so: reset every other one)
            mask = term & (np.arange(B) % 2 == 0)
            o1, i1 = env.reset(mask=mask)
            lockstep.same_obs(o1, orc.reset(mask=mask.astype(np.uint8)), "masked reset obs", t)
            met.update(same_mask(env, orc, "masked reset", i1))
            met["reset"] += int(mask.sum())

    lockstep.lockstep(env, orc, actions, mode, seed=None, steps=STEPS, on_step=on_step)
    print({k: met[k] for k in CASES})
    assert all(met[k] > 0 for k in CASES), f"the run never met {[k for k in CASES if not met[k]]}: it proves nothing"
    env.close()


# (env id, constructor extras, envs, env keywords): the smallest shapes at which each kernel path exists
TINY4 = ("rware-tiny-4ag-v1", {}, 32, {})                                            # exact shape, DPP exchange; two workgroups
TINY9 = ("rware-tiny-9ag-v1", {}, 16, {})                                            # per-cell exchange (kCell)
SMALL16 = ("rware-small-16ag-v1", {}, 16, {})                                        # two agent wavefronts per workgroup
SHAPES = [
    ("rware-tiny-2ag-v1", {}, 19, {"envs_per_workgroup": 4, "threads_per_workgroup": 64}),   # the generic kernel, a ragged last workgroup
    TINY4, TINY9, SMALL16,
    ("rware-small-4ag-v1", {"n_agents": 20}, 8, {}),                                 # 20 agents: the LDS agent phases
    ("rware-tiny-3ag-v1", {"sensor_range": 2}, 16, {}),
    ("rware-tiny-2ag-v1", {"msg_bits": 2}, 16, {}),
    ("rware-img-tiny-3ag-v1", {}, 16, {}),                                           # IMAGE
    ("rware-imgdict-tiny-2ag-v1", {}, 16, {}),                                       # IMAGE_DICT
]
RUNS = [(s, m) for s in SHAPES for m in MODES]
RUN_IDS = [f"{s[0]}{''.join(f'-{k}{v}' for k, v in s[1].items())}-{m}" for s, m in RUNS]


# ------------------------------------------------------------------------------------------------------------------------------
# the shared checks: the library is the only difference between the CPU and the GPU suite
# ------------------------------------------------------------------------------------------------------------------------------
def check_constructed(lib, jit=None):
    """tiny warehouse, two agents, one scenario per env: the rare cases random play meets ~3 times per run, and the four corners"""
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1")
    corners = [(cx, cy, d) for cx in (0, 9) for cy in (0, 10) for d in range(4)]
    corners = (2 * corners)[:29]                             # (32 envs in all: a batch every exact-shape workgroup geometry divides)
    B = 3 + len(corners)
    env, orc = make_env(lib, kw, B, jit=jit), OracleVecEnv(B, **kw)
    env.reset(seed=3)
    orc.reset(seed=3)
    assert (orc.H, orc.W) == (11, 10) and orc.hw[1, 1] == 0 and orc.hw[0, 1] and orc.hw[1, 0]
    # shelves back on their home cells, in id order (np.nonzero order of the shelf cells), whatever the reset state was
    ys, xs = np.nonzero(orc.hw == 0)
    sxy = np.tile(np.stack([xs, ys], -1).astype(np.int32), (B, 1, 1))
    sid = {(int(x_), int(y_)): k + 1 for k, (x_, y_) in enumerate(zip(xs, ys))}
    f = {k: np.zeros((B, 2), np.int32) for k in ("agent_x", "agent_y", "agent_dir", "agent_carry", "agent_delivered")}
    # envs 0..2: the subject (agent 0) on the highway cell (0, 1) facing RIGHT, the occupant (agent 1) on the shelf cell (1, 1) heading UP
    # to the empty highway cell (1, 0)
    f["agent_x"][:3], f["agent_y"][:3], f["agent_dir"][:3] = (0, 1), (1, 1), (RIGHT, UP)
    spare = sid[(8, 8)]                                      # the shelf the subject carries, where it does
    for e in (0, 1):
        f["agent_carry"][e, 0] = spare
        sxy[e, spare - 1] = (0, 1)
    f["agent_carry"][1, 1] = sid[(1, 1)]                     # env 1: the occupant carries the shelf of its cell
    #   env 0: loaded, facing an UNLOADED agent under a shelf: cancel;  env 1: loaded facing loaded: no cancel;  env 2: unloaded facing an agent
    for k, (cx, cy, d) in enumerate(corners):                # envs 3..: agent 0 in a corner in every heading, agent 1 out of the way
        e = 3 + k
        f["agent_x"][e], f["agent_y"][e], f["agent_dir"][e] = (cx, 4), (cy, 5), (d, UP)
    for who in (env, orc):
        who.set_state(**f) if who is orc else who.set_state(refresh_obs=False, **f)
        who.recalc_grid(sxy)                                 # (the env: refreshes the observation and with it the mask)
    lockstep.same_state(env.get_state(), orc.get_state(), "constructed")
    same_mask(env, orc, "constructed")
    model_matches_probe(orc, kw, "constructed")
    got = raw_bytes(env)
    assert [int(got[e, 0]) & 0x22 for e in range(3)] == [0x00, 0x20, 0x20], got[:3, 0]
    for k, (cx, cy, d) in enumerate(corners):
        out = (d == UP and cy == 0) or (d == DOWN and cy == 10) or (d == LEFT and cx == 0) or (d == RIGHT and cx == 9)
        assert (int(got[3 + k, 0]) & 0x22) == (0 if out else 2), (cx, cy, d, got[3 + k, 0])
    # bit 5, operationally: both agents FORWARD, the occupant leaves — the follower moves iff bit 5
    before = (orc.agent_x[:3, 0].copy(), orc.agent_y[:3, 0].copy())
    a = np.zeros((B, 2), np.int32)
    a[:3] = FORWARD
    env.step(a)
    orc.step(a)
    assert (orc.agent_x[:3, 1] == 1).all() and (orc.agent_y[:3, 1] == 0).all(), "the occupant did not leave"
    moved = (orc.agent_x[:3, 0] != before[0]) | (orc.agent_y[:3, 0] != before[1])
    assert moved.tolist() == [False, True, True] and moved.tolist() == [bool(got[e, 0] & 0x20) for e in range(3)]
    lockstep.same_state(env.get_state(), orc.get_state(), "constructed, one step on")
    same_mask(env, orc, "constructed, one step on")
    env.close()


def check_rollout(lib, env_id, B, mode, jit=None, T=30):
    """a fused launch of T steps leaves the mask of its last step == T single steps; three more single steps carry on"""
    kw = lockstep.oracle_kwargs(env_id, max_steps=MAX_STEPS)
    env, single, orc = make_env(lib, kw, B, mode, jit), make_env(lib, kw, B, mode, jit), OracleVecEnv(B, **kw)
    for who in (env, single, orc):
        who.reset(seed=5)
    acts = np.random.default_rng(1).choice(5, size=(T + 3, B, kw["n_agents"]), p=P_ACT).astype(np.int32)
    _, _, term = env.rollout(acts[:T], want_obs=False)
    for t in range(T):
        single.step(acts[t])
        orc.step_autoreset(acts[t], mode)
    assert np.asarray(term).any(), "no episode ended inside the launch"
    assert np.array_equal(raw_bytes(env), raw_bytes(single))
    same_mask(env, orc, (mode, "after the rollout"))
    for t in range(T, T + 3):
        info = env.step(acts[t])[4]
        orc.step_autoreset(acts[t], mode)
        same_mask(env, orc, (mode, t), info)
    env.close()
    single.close()


def check_state_forms(lib, jit=None):
    """masked reset, set_state + refresh, snapshot / restore: every launch that writes an observation writes the mask"""
    B = 32
    kw = lockstep.oracle_kwargs("rware-tiny-4ag-v1", max_steps=MAX_STEPS)
    env, orc = make_env(lib, kw, B, jit=jit), OracleVecEnv(B, **kw)
    env.reset(seed=4)
    orc.reset(seed=4)
    acts = np.random.default_rng(6).choice(5, size=(24, B, 4), p=P_ACT).astype(np.int32)

    def run(t0, t1):
        for t in range(t0, t1):
            env.step(acts[t])
            orc.step_autoreset(acts[t], "next_step")

    run(0, 8)
    same_mask(env, orc, "8 steps")
    mask = np.arange(B) % 3 == 0
    _, info = env.reset(mask=mask)
    orc.reset(mask=mask.astype(np.uint8))
    same_mask(env, orc, "masked reset", info)                # (the envs outside the mask: the mask of their current state)
    run(8, 12)
    new_dir = (orc.agent_dir + 1) % 4                        # set_state + refresh: every agent turned
    stale = raw_bytes(env)
    env.set_state(refresh_obs=False, agent_dir=new_dir)
    orc.set_state(agent_dir=new_dir)
    assert np.array_equal(raw_bytes(env), stale)             # (an output of the launches: a state write alone does not touch it)
    env.set_state(agent_dir=new_dir)                         # ... the refresh does
    same_mask(env, orc, "set_state + refresh")
    assert not np.array_equal(raw_bytes(env), stale)
    snap, before, st, pending = env.snapshot(), raw_bytes(env), orc.get_state(), orc._prev_done.copy()
    run(12, 24)
    later = raw_bytes(env)
    same_mask(env, orc, "24 steps")
    assert not np.array_equal(later, before)
    env.restore(snap)
    assert np.array_equal(raw_bytes(env), before)
    orc.set_state(**st)
    orc._prev_done[:] = pending
    run(12, 24)
    assert np.array_equal(raw_bytes(env), later)
    env.free_snapshot(snap)
    env.close()


def check_shards(lib):
    B = 24
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1", max_steps=MAX_STEPS)
    env, orc = make_env(lib, kw, B, devices=[0, 0]), OracleVecEnv(B, **kw)
    assert len(env.engines) == 2
    rng = np.random.default_rng(9)
    _, info = env.reset(seed=3)
    orc.reset(seed=3)
    same_mask(env, orc, "sharded reset", info)
    for t in range(30):
        a = rng.choice(5, size=(B, 2), p=P_ACT).astype(np.int32)
        info = env.step(a)[4]
        orc.step_autoreset(a, "next_step")
        same_mask(env, orc, ("sharded", t), info)
    env.close()


def check_combination(lib, jit=None):
    """RW_STATS_ON | RW_EPISODES_ON | RW_OBS_PACKED | RW_ACTION_MASK_ON on one engine: everything holds"""
    B = 32
    kw = lockstep.oracle_kwargs("rware-tiny-4ag-v1", max_steps=9)
    env = make_env(lib, kw, B, jit=jit, stats=True, episode_stats=True, obs_format="packed")
    assert env.engines[0].info.stats == 7
    orc = OracleVecEnv(B, **kw)
    rng = np.random.default_rng(3)
    obs, info = env.reset(seed=2)
    assert np.array_equal(env.unpack_obs(obs), orc.reset(seed=2))
    same_mask(env, orc, "reset", info)
    ends = 0
    for t in range(24):
        a = rng.choice(5, size=(B, 4), p=P_ACT).astype(np.int32)
        obs, rew, term, _, info = env.step(a)
        o2, r2, d2 = orc.step_autoreset(a, "next_step")
        assert np.array_equal(env.unpack_obs(obs), o2) and np.array_equal(rew, r2) and np.array_equal(term, d2.astype(bool)), t
        same_mask(env, orc, t, info)
        assert ("episode" in info) == bool(d2.any())
        ends += int(d2.sum())
    c = env.event_counters()
    assert np.array_equal(c["failed_moves"], orc.stat_failed_moves) and np.array_equal(c["deliveries"], orc.stat_deliveries)
    assert ends >= B and np.array_equal(env.episode_stats()["count"], np.full(B, ends // B, np.int32))
    env.close()


def check_off_switch(lib):
    B = 16
    kw = lockstep.oracle_kwargs("rware-tiny-4ag-v1", max_steps=6)
    off = rware_amd.WarehouseVecEnv(B, library=lib, **kw)
    on = make_env(lib, kw, B)
    eng = off.engines[0]
    assert eng.action_mask is False and not eng.info.stats & 4 and on.engines[0].info.stats == 4
    C = rware_amd._capi.C
    nbytes = C.c_size_t(7)
    eng._check(eng.lib.rw_get_buffer(eng._h, rware_amd._capi.BUF["action_mask"], None, C.byref(nbytes)))
    assert nbytes.value == 0
    on.engines[0]._check(on.engines[0].lib.rw_get_buffer(on.engines[0]._h, 28, None, C.byref(nbytes)))
    assert nbytes.value == B * 4
    with pytest.raises(RuntimeError, match="action_mask=True"):
        off.action_mask()
    with pytest.raises(rware_amd._capi.EngineError):          # an empty buffer: reading B * N bytes from it is refused
        eng.read("action_mask")
    with pytest.raises(rware_amd._capi.EngineError, match="read-only"):   # rw_write refuses it, with the flag ...
        on.engines[0].write("action_mask", np.zeros((B, 4), np.uint8))
    with pytest.raises(rware_amd._capi.EngineError, match="read-only"):   # ... and without (0 bytes offered to the empty buffer)
        eng._check(eng.lib.rw_write(eng._h, 28, None, 0))
    a, b = eng.info, on.engines[0].info
    # (which kernel runs may differ — the ahead-of-time builds do not carry the code — the workgroups and their LDS do not)
    assert (a.envs_per_workgroup, a.n_workgroups, a.lds_bytes) == (b.envs_per_workgroup, b.n_workgroups, b.lds_bytes)
    assert b.engine_bytes_per_env_step == a.engine_bytes_per_env_step + 4
    o0, i0 = off.reset(seed=8)
    o1, i1 = on.reset(seed=8)
    assert np.array_equal(o0, o1) and i0 == {} and set(i1) == {"action_mask"}
    acts = np.random.default_rng(2).choice(5, size=(14, B, 4), p=P_ACT).astype(np.int32)
    for t in range(14):                                       # the mask changes nothing else (episodes end on the way: max_steps 6)
        x, y = off.step(acts[t]), on.step(acts[t])
        assert all(np.array_equal(p, q) for p, q in zip(x[:4], y[:4])), t
        assert x[4] == {} and set(y[4]) == {"action_mask"}
    s0, s1 = off.get_state(), on.get_state()
    assert set(s0) == set(s1) and all(np.array_equal(v, s1[k]) for k, v in s0.items())   # (an output, not state)
    off.close()
    on.close()


def check_pipe_fallback(lib):
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    env = rware_amd.WarehouseVecEnv(32, library=lib, action_mask=True, pipe=True, **kw)
    assert env.engines[0].info.pipe_workgroups == 0 and "RW_ACTION_MASK_ON" in env.engines[0].jit_log()
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------
# CPU suite: the product sources on host threads
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(1500)
@pytest.mark.parametrize("shape,mode", RUNS, ids=RUN_IDS)
def test_emulated_mask_matches_the_model_and_the_solo_probe(shape, mode):
    env_id, extra, B, env_kw = shape
    check_lockstep(emu_library(), env_id, extra, B, mode, **env_kw)


@pytest.mark.timeout(1500)
def test_emulated_constructed_states_and_the_follow_chain_bit():
    check_constructed(emu_library())


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_fused_rollout_leaves_the_mask_of_its_last_step(mode):
    check_rollout(emu_library(), "rware-tiny-4ag-v1", 32, mode)


@pytest.mark.timeout(1500)
def test_emulated_masked_reset_state_writes_and_snapshots():
    check_state_forms(emu_library())


@pytest.mark.timeout(1500)
def test_emulated_sharded_env_gathers_the_mask_in_env_order():
    check_shards(emu_library())


@pytest.mark.timeout(1500)
def test_emulated_mask_combines_with_counters_episode_statistics_and_packed_rows():
    check_combination(emu_library())


@pytest.mark.timeout(1500)
def test_emulated_off_switch_read_only_and_info_bit():
    check_off_switch(emu_library())


@pytest.mark.timeout(1500)
def test_emulated_pipelined_request_falls_back_to_the_classic_kernel():
    check_pipe_fallback(emu_library())


# ------------------------------------------------------------------------------------------------------------------------------
# GPU suite: the gfx950 library, through the C-ABI
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", RUNS, ids=RUN_IDS)
def test_mask_matches_the_model_and_the_solo_probe_generic_kernels(shape, mode):
    env_id, extra, B, env_kw = shape
    check_lockstep(None, env_id, extra, B, mode, **env_kw)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [TINY4, TINY9, SMALL16], ids=lambda s: s[0])
def test_mask_matches_the_model_and_the_solo_probe_run_time_exact_shape_builds(shape, mode):
    env_id, extra, B, env_kw = shape
    check_lockstep(None, env_id, extra, B, mode, jit="force", **env_kw)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [None, "force"])
def test_constructed_states_and_the_follow_chain_bit(jit):
    check_constructed(None, jit)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("jit", [None, "force"])
def test_fused_rollout_leaves_the_mask_of_its_last_step(jit, mode):
    check_rollout(None, "rware-tiny-4ag-v1", 32, mode, jit)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [None, "force"])
def test_masked_reset_state_writes_and_snapshots(jit):
    check_state_forms(None, jit)


@pytest.mark.gpu
def test_sharded_env_gathers_the_mask_in_env_order():
    check_shards(None)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [None, "force"])
def test_mask_combines_with_counters_episode_statistics_and_packed_rows(jit):
    check_combination(None, jit)


@pytest.mark.gpu
def test_off_switch_read_only_and_info_bit():
    check_off_switch(None)


@pytest.mark.gpu
def test_pipelined_request_falls_back_to_the_classic_kernel():
    check_pipe_fallback(None)


@pytest.mark.gpu
def test_an_engine_with_the_mask_gets_a_kernel_that_writes_it(tmp_path, monkeypatch):
    """rw_create's choice, as for the event counters: the generic kernel below 4096 envs, a run-time compiled exact-shape build from
    there on (rw_jit_log says why)"""
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    big = rware_amd.WarehouseVecEnv(4096, action_mask=True, **kw)
    j = big.engines[0].info
    assert (j.stats, j.jit, j.build_kind, j.specialised) == (4, 1, 1, 1), big.engines[0].jit_log()
    assert "action masks" in big.engines[0].jit_log()
    small = rware_amd.WarehouseVecEnv(64, action_mask=True, **kw)
    k = small.engines[0].info
    assert (k.stats, k.jit, k.build_kind) == (4, 0, 0)
    big.close()
    small.close()


@pytest.mark.gpu
def test_the_zero_copy_mask_is_current_inside_a_captured_loop():
    """output="torch": the policy of a captured loop copies the zero-copy uint8 (B, N) tensor into a (T, B, N) record — what a masked
    policy would sample with at every replayed step — and the record equals the model of the oracle's state in front of each step"""
    import torch

    B, N, K = 64, 4, 12
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1", max_steps=5)
    env = rware_amd.WarehouseVecEnv(B, output="torch", action_mask=True, **kw)
    orc = OracleVecEnv(B, **kw)
    _, info = env.reset(seed=31)
    orc.reset(seed=31)
    assert info == {}                                         # torch output: no host synchronisation, no keys
    raw = env.device_tensor("action_mask")
    assert raw.is_cuda and raw.dtype == torch.uint8 and raw.shape == (B, N) and raw.data_ptr() == env.engines[0].device_array("action_mask").ptr
    tape = np.random.default_rng(4).choice(5, size=(K, B, N), p=P_ACT).astype(np.int32)
    dev_tape = torch.from_numpy(tape).cuda()
    cursor = torch.zeros((), dtype=torch.long, device="cuda")
    record = torch.zeros((K, B, N), dtype=torch.uint8, device="cuda")

    def policy(obs, rewards, terminated):                     # capturable: record the mask this step's actions answer, play the tape
        record.index_copy_(0, cursor.reshape(1), raw.unsqueeze(0))
        a = dev_tape.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return a

    loop = env.capture_loop(policy, steps=K, warmup=0)
    cursor.zero_()
    record.zero_()
    loop.replay()
    torch.cuda.synchronize()
    got, ends = record.cpu().numpy(), 0
    for t in range(K):
        want, _ = mask_model(orc.get_state(), orc.hw)
        assert np.array_equal(got[t], want), t
        ends += int(orc.step_autoreset(tape[t], "next_step")[2].sum())
    assert ends >= B
    want, _ = mask_model(orc.get_state(), orc.hw)
    assert np.array_equal(raw.cpu().numpy(), want)
    m, mp = env.action_mask(), env.action_mask(permissive=True)
    assert m.is_cuda and m.dtype == torch.bool and m.shape == (B, N, 5)
    assert np.array_equal(m.cpu().numpy(), bits(want)) and np.array_equal(mp.cpu().numpy(), bits(want, True))
    assert env.step(dev_tape[0])[4] == {}
    env.close()


@pytest.mark.gpu
def test_two_pipelines_carry_the_mask_of_their_sub_batches():
    import torch

    B, N = 64, 4
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1", max_steps=MAX_STEPS)
    pipes = rware_amd.make_pipelines(B, 2, action_mask=True, **{k: v for k, v in rware_amd.env_kwargs("rware-small-4ag-v1").items()
                                                                 if k != "max_steps"}, max_steps=MAX_STEPS)
    orc = OracleVecEnv(B, **kw)
    orc.reset(seed=11)
    for p in pipes:
        p.reset(seed=11)
    rng = np.random.default_rng(2)
    for t in range(30):
        a = rng.choice(5, size=(B, N), p=P_ACT).astype(np.int32)
        for p in pipes:
            with p as env:
                env.step(torch.from_numpy(a[p.lo:p.hi]).cuda())
        orc.step_autoreset(a, "next_step")
    want, _ = mask_model(orc.get_state(), orc.hw)
    for p in pipes:
        p.stream.synchronize()
        assert np.array_equal(p.env.device_tensor("action_mask").cpu().numpy(), want[p.lo:p.hi])
        assert np.array_equal(p.env.action_mask().cpu().numpy(), bits(want[p.lo:p.hi]))
        p.env.close()
