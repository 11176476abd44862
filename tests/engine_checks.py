"""Oracle-parity checks that the emulated suite (tests/test_engine_emulated.py: the kernels on host threads) and the device suite
(tests/test_gpu_parity.py) run with the same body and their own sizes.  Every body goes through lockstep.lockstep / check_rollout;
what is specific to a check (rw_info assertions, counters, the census) stays beside its call."""
from collections import Counter

import numpy as np

import rware_amd
from lockstep import attempt, check_rollout, lockstep, oracle_kwargs, same_state
from rware_oracle import OracleVecEnv

P_DEFAULT = [.1, .55, .1, .1, .15]


def default_envs_per_workgroup(task, N):
    # the table's rule for small batches (csrc/rware_static_table.h): 16 envs up to 4 agents, 8 from 5 on; 9 .. 19 agents on the small
    # warehouse step on 4-env workgroups below one round of them and roll out on 8 (13 .. 16 agents), the tiny one has 8-env builds only
    return 16 if N <= 4 else 4 if task.startswith("small") and N >= 9 else 8


def square(max_steps):
    """A 10 x 10 grid: the transposed index of the AGENT_DIRECTION / AGENT_LOAD layers is always in bounds."""
    return dict(shelf_columns=3, column_height=3, shelf_rows=2, n_agents=5, msg_bits=0, sensor_range=2,
                request_queue_size=3, max_inactivity_steps=None, max_steps=max_steps, reward_type=1)


def make_pair(B, kw, *, library=None, geom=(0, 0), **env_only):
    """The env (this library, this geometry) and the oracle from ONE dict of constructor arguments."""
    env = rware_amd.WarehouseVecEnv(B, library=library, envs_per_workgroup=geom[0], threads_per_workgroup=geom[1], **env_only, **kw)
    return env, OracleVecEnv(B, **kw)


def image_observations(kw, B, *, tape_steps, n_step, library=None, geom=(0, 0)):
    """IMAGE / IMAGE_DICT observations: `n_step` per-step launches, then the rest of the tape as one fused rollout (the image tape)."""
    env, orc = make_pair(B, kw, library=library, geom=geom)
    acts = np.random.default_rng(7).choice(5, size=(tape_steps, B, kw["n_agents"]), p=[.1, .5, .15, .15, .1])
    lockstep(env, orc, acts[:n_step], seed=4)
    if n_step < tape_steps:
        check_rollout(env, orc, acts[n_step:], t0=n_step)      # fused rollout writes the image tape
    env.close()


def transposed_image_layers(extra, layers, B, *, max_steps, seed, rng_seed, tape_steps, n_step, library=None, geom=(0, 0)):
    """AGENT_DIRECTION / AGENT_LOAD as the reference writes them, layer[ag.x, ag.y] (:552, :558), on the square grid; per-step
    launches and a fused rollout."""
    env, orc = make_pair(B, dict(square(max_steps), **extra), library=library, geom=geom)
    assert tuple(env.grid_size) == (10, 10)
    acts = np.random.default_rng(rng_seed).choice(5, size=(tape_steps, B, 5), p=[.1, .45, .15, .15, .15])
    seen = Counter()

    def count(t, o, r, d, info):
        img = o["image"] if isinstance(o, dict) else o
        seen["dir"] += int((img[:, :, layers.index(3)] > 1).sum())
        seen["load"] += int(img[:, :, layers.index(4)].sum())

    lockstep(env, orc, acts[:n_step], seed=seed, on_step=count)
    assert seen["dir"] > 0 and seen["load"] > 0          # the layers were exercised (values 2..4, loaded agents in view)
    check_rollout(env, orc, acts[n_step:], t0=n_step)
    env.close()


def transposed_layers_raise_indexerror(env_id, layer, B, *, limit, library=None, geom=(0, 0)):
    """H > W on every registered layout: the reference's layer[ag.x, ag.y] raises IndexError once an agent (a loaded one for
    AGENT_LOAD) reaches y >= W; the engine reports it for the same reset() / step() call."""
    kw = oracle_kwargs(env_id, observation_type=2, image_observation_layers=[2, layer])
    env, orc = make_pair(B, kw, library=library, geom=geom)
    rng = np.random.default_rng(1)
    (o, e1), (o2, e2) = attempt(lambda: env.reset(seed=2)[0]), attempt(lambda: orc.reset(seed=2))
    assert e1 == e2
    t = 0
    while not e1 and t < limit:
        a = rng.choice(5, size=(B, kw["n_agents"]), p=[.05, .5, .15, .15, .15])
        (res, e1), (res2, e2) = attempt(lambda: env.step(a)), attempt(lambda: orc.step_autoreset(a, "next_step"))
        assert e1 == e2, t
        if not e1:
            assert np.array_equal(res[0], res2[0]), t
        t += 1
    assert e1, "no agent ever reached y >= W"
    env.close()


def random_shape(kw, B, mode, geom, *, case, seed, n_step, n_roll, library=None):
    """The generic kernel on one drawn warehouse: per-step launches across autoresets (autoreset disabled: the ended envs reset by
    mask) and, where the engine resets on its own, a fused rollout."""
    env, orc = make_pair(B, kw, library=library, geom=geom, autoreset_mode=mode)
    rng = np.random.default_rng(case)
    draw = lambda *lead: rng.choice(5, size=lead + (B, kw["n_agents"]), p=P_DEFAULT).astype(np.int32)

    def reset_ended(t, obs, rew, term, info):
        if mode == "disabled" and term.any():
            m = term.astype(np.uint8)
            assert np.array_equal(env.reset(mask=m)[0], orc.reset(mask=m)), (t, kw)

    try:
        lockstep(env, orc, lambda t: draw(), mode, seed=seed, steps=n_step, on_step=reset_ended)
        acts = draw(n_roll)
        if mode != "disabled":
            check_rollout(env, orc, acts, mode, t0=n_step)
        same_state(env.get_state(), orc.get_state(), "end")     # (autoreset disabled: after the last reset by mask)
    except AssertionError as e:
        raise AssertionError(f"{e} — {kw}, B={B}, geometry {geom}") from e
    env.close()


def crowded_warehouse(env_id, p_forward, B, *, max_steps, n_step, envs_per_workgroup, census=0, library=None, geom=(0, 0)):
    """A forward-heavy policy on a crowded warehouse: the per-cell agent phases of the per-step kernel, then the register-exchange
    ones of the fused rollout.  `census`: how many envs' pre-step states go through collision_scenarios.analyse (printed)."""
    kw = oracle_kwargs(env_id, max_steps=max_steps)
    N = kw["n_agents"]
    env, orc = make_pair(B, kw, library=library, geom=geom)
    assert env.engines[0].info.build_kind == 2 and env.engines[0].info.envs_per_workgroup == envs_per_workgroup
    rng = np.random.default_rng(33)
    rest = (1.0 - p_forward) / 4
    seen = Counter()

    def act(t):
        a = rng.choice(5, size=(B, N), p=[rest, p_forward, rest, rest, rest]).astype(np.int32)
        if census:                                       # what this step is made of: the oracle's pre-step state
            import collision_scenarios as cs
            so = orc.get_state()
            for e in range(census):
                seen.update(cs.analyse(so["agent_x"][e], so["agent_y"][e], so["agent_dir"][e], so["agent_carry"][e], a[e], orc.H, orc.W, so["grid"][e, 1])[0])
        return a

    lockstep(env, orc, act, seed=31, steps=n_step)
    if census:
        print(f"census {env_id} ({census} envs x {n_step} steps): {dict(sorted(seen.items()))}")
        assert seen
    acts = rng.choice(5, size=(25, B, N), p=[rest, p_forward, rest, rest, rest]).astype(np.int32)
    check_rollout(env, orc, acts, t0=n_step)             # the fused rollout keeps the all-gather (register) agent phases
    env.close()


def steps_interleaved_with_rollouts(cases, *, max_steps, seed, rng_seed, n_step, n_roll, rollout_obs, library=None):
    """9 .. 19 agents on the 4-env per-step build: per-step launches and fused rollouts (another geometry of the same engine) in turn,
    two rounds, each on the state the other left."""
    for env_id, B in cases:
        kw = oracle_kwargs(env_id, max_steps=max_steps)
        N = kw["n_agents"]
        env, orc = make_pair(B, kw, library=library)
        assert env.engines[0].info.envs_per_workgroup == 4
        rng = np.random.default_rng(rng_seed)
        draw = lambda *lead: rng.choice(5, size=lead + (B, N), p=P_DEFAULT).astype(np.int32)
        t = 0
        try:
            for rnd in range(2):
                lockstep(env, orc, lambda t: draw(), seed=seed if rnd == 0 else None, steps=n_step, t0=t)
                check_rollout(env, orc, draw(n_roll), t0=t + n_step, want_obs=rollout_obs)
                t += n_step + n_roll
        except AssertionError as e:
            raise AssertionError(f"{env_id}: {e}") from e
        env.close()


def image_terminal_observations(kw, B, *, steps, seed, library=None, geom=(0, 0)):
    """SAME_STEP autoreset with IMAGE / IMAGE_DICT observations: observations, rewards, flags every step and the terminal observation
    of every env that ended an episode (info["final_obs"], rows info["_final_obs"]).  Returns how many of those were compared."""
    env, orc = make_pair(B, kw, library=library, geom=geom, autoreset_mode="same_step")
    rng = np.random.default_rng(3)
    run = lockstep(env, orc, lambda t: rng.choice(5, size=(B, kw["n_agents"]), p=P_DEFAULT).astype(np.int32), "same_step",
                   seed=seed, steps=steps)
    env.close()
    return run.finals
