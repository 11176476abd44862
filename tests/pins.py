"""What every constructed pin does (collisions, PCG64 draws, observation windows, shelf handling, more than 64 agents): scenarios built
by hand, recorded from the unmodified reference into tests/golden/<dir>/ by its generate_*.py, replayed on the oracle, the emulated
kernels and every GPU kernel path.  Plain functions: a pin supplies its scenarios, its generator, the `fields` its fixture records and
a `name_of(task, z, k, t)` that names scenario k at step t in a failure message.  A fixture `z` is the dict `load_npz` hands out: the
injected state under its field names, what the reference recorded behind step t under r_<field>[scenario, t], `meta` parsed.
"""
import glob
import importlib.util
import json
import os

import numpy as np

AGENT_FIELDS = ("agent_x", "agent_y", "agent_dir", "agent_carry", "agent_delivered")
STATE_FIELDS = AGENT_FIELDS + ("shelf_xy", "queue", "agent_msg", "steps", "inactive", "rng")
_cache = {}


# ------------------------------------------------------------------------------------------------------------------ fixtures
def load_npz(fix_dir, task, prepare=None):
    """<fix_dir>/<task>.npz as a dict, loaded once per `prepare`: `meta` parsed, `prepare(z)` applied (the pin's own part: observations
    unpacked, a field the generator does not store — a module-level function, it is part of the cache key), every array read-only."""
    named = getattr(prepare, "__qualname__", "<locals>")      # (a nested function, a lambda or a partial is a new cache key at every call)
    assert prepare is None or not ("<locals>" in named or "<lambda>" in named), f"`prepare` must be a module-level function: {prepare}"
    key = (fix_dir, task, prepare)
    if key not in _cache:
        z = dict(np.load(os.path.join(fix_dir, f"{task}.npz")))
        z["meta"] = json.loads(str(z["meta"]))
        if prepare is not None:
            prepare(z)
        for a in z.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = z
    return _cache[key]


def load_generator(path):
    """A generate_*.py of tests/golden/ as a module (they are scripts in directories that are no packages)."""
    spec = importlib.util.spec_from_file_location(os.path.basename(path)[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_fixture_directory_is_small(fix_dir, tasks, limit=2_000_000):
    """The size rule of a fixture directory: one .npz per task, under `limit` bytes in all, none larger than the largest golden trace."""
    files = glob.glob(os.path.join(fix_dir, "*.npz"))
    assert sorted(os.path.basename(f)[:-4] for f in files) == sorted(tasks)
    golden = os.path.dirname(fix_dir)
    largest_other = max(os.path.getsize(f) for f in glob.glob(os.path.join(golden, "*.npz")))
    assert sum(os.path.getsize(f) for f in files) < limit and max(os.path.getsize(f) for f in files) <= largest_other


def assert_regenerates(fresh_path, committed_path):
    """What the generator wrote just now is the committed fixture: the same arrays, dtype and bytes."""
    fresh, z = dict(np.load(fresh_path)), dict(np.load(committed_path))
    assert sorted(fresh) == sorted(z)
    for k in z:
        assert fresh[k].dtype == z[k].dtype and fresh[k].tobytes() == z[k].tobytes(), (committed_path, k)


def pad_batch(idx, multiple, ragged=False, fill=0):
    """idx padded with copies of scenario `fill` to a whole number of `multiple` envs — `ragged`: one more, a partial last workgroup."""
    idx = np.asarray(idx)
    pad = (-len(idx)) % multiple + (1 if ragged else 0)
    return np.concatenate([idx, np.full(pad, fill, idx.dtype)])


# ------------------------------------------------------------------------------------------------------------------ injection
def inject_reference(env, sc, rng_state=None, counters=False):
    """One scenario (agent_x / agent_y / agent_dir / agent_carry (N,), shelf_xy (S, 2), queue (Q,)) into a reference env, the way the
    reference's own tests do it: overwrite the objects, `_recalc_grid()`.  Flags and both counters are zeroed or, `counters`, taken
    from the scenario's agent_delivered / steps / inactive.  `rng_state`: numpy's bit-generator state."""
    import ref_runner as rr
    wh = rr.load_reference()
    for i, ag in enumerate(env.agents):
        ag.x, ag.y, ag.dir = int(sc["agent_x"][i]), int(sc["agent_y"][i]), wh.Direction(int(sc["agent_dir"][i]))
        c = int(sc["agent_carry"][i])
        ag.carrying_shelf = env.shelfs[c - 1] if c else None
        ag.has_delivered = bool(sc["agent_delivered"][i]) if counters else False
    for s, (x, y) in zip(env.shelfs, sc["shelf_xy"]):
        s.x, s.y = int(x), int(y)
    env.request_queue = [env.shelfs[int(q) - 1] for q in sc["queue"]]
    env._cur_steps, env._cur_inactive_steps = (int(sc["steps"]), int(sc["inactive"])) if counters else (0, 0)
    if rng_state is not None:
        env.np_random.bit_generator.state = rng_state
    env._recalc_grid()


def _is_oracle(be):
    from rware_oracle import OracleVecEnv      # (here: tests/wide_fixtures.py loads through this module and needs no oracle)
    return isinstance(be, OracleVecEnv)


def write_state(be, fields, shelf_xy):
    """State fields and every shelf's cell into an oracle or an engine; returns the observation of that state."""
    if _is_oracle(be):
        be.set_state(**fields)
        be.recalc_grid(shelf_xy)
        return be.obs()
    be.set_state(refresh_obs=False, **fields)
    be.recalc_grid(shelf_xy)
    return be.observations()


def inject(be, z, idx):
    """Scenarios `idx` of the fixture into the B = len(idx) envs of an oracle or an engine, behind a reset with the fixture's seed."""
    B = len(idx)
    fields = {f: z[f][idx].astype(np.int32) for f in AGENT_FIELDS}
    fields["queue"] = z["queue"][idx].astype(np.int32)
    fields["rng"] = z["rng"][idx] if "rng" in z else np.repeat(z["rng0"][None], B, axis=0)     # (one state per scenario, or the reset's)
    fields.update({f: z[f][idx].astype(np.int32) for f in ("steps", "inactive") if f in z})
    seed = z["meta"]["seed"]
    be.reset(seed=seed if _is_oracle(be) else [seed] * B)
    return write_state(be, fields, np.ascontiguousarray(z["shelf_xy"][idx].astype(np.int32)))


# ------------------------------------------------------------------------------------------------------------------ checks
def _first_env(got, want):
    return int(np.argwhere((got != want).reshape(len(got), -1).any(-1))[0, 0])


def check_state(task, z, idx, t, state, shelf_xy, rew=None, done=None, who="", *, fields, name_of):
    """The recorded `fields` of step t, then rewards and done, for the scenarios idx against what a backend holds; names the first miss."""
    assert set(fields) <= set(STATE_FIELDS), fields

    def fail(e, what):
        raise AssertionError(f"{who}{name_of(task, z, int(idx[e]), t)}: {what}")

    for f in fields:
        got, want = np.asarray(shelf_xy if f == "shelf_xy" else state[f]), z["r_" + f][idx, t]
        if f == "rng":
            got = got.astype(np.uint64)
        if np.array_equal(got, want):
            continue
        if f in AGENT_FIELDS:
            e, i = [int(v) for v in np.argwhere(got != want)[0]]
            k = int(idx[e])
            prev = z[f][k] if t == 0 else z["r_" + f][k, t - 1]
            verb = "moved" if f in ("agent_x", "agent_y") and want[e, i] == prev[i] else \
                "did not move" if f in ("agent_x", "agent_y") and got[e, i] == prev[i] else "differs"
            fail(e, f"agent {i} {verb}: {f} = {int(got[e, i])}, reference {int(want[e, i])} (was {int(prev[i])})")
        elif f == "agent_msg":
            e, i = [int(v) for v in np.argwhere(got != want)[0]]
            fail(e, f"agent {i}: {f} = {int(got[e, i])}, reference {int(want[e, i])}")
        elif f == "shelf_xy":
            e, s = [int(v) for v in np.argwhere((got != want).any(-1))[0]]
            fail(e, f"shelf {s + 1} at {got[e, s].tolist()}, reference {want[e, s].tolist()}")
        else:
            e = _first_env(got, want)
            hint = " (the replacement draws follow the goal list's order)" if f == "queue" else ""
            fail(e, f"{f} {got[e].tolist()}, reference {want[e].tolist()}{hint}")
    check_rewards(task, z, idx, t, rew, done, who, name_of=name_of)


def check_rewards(task, z, idx, t, rew, done, who="", *, name_of):
    """Rewards (x 2 in the fixture: TWO_STAGE halves stay integers) and done of step t; None: not compared."""
    def fail(e, what):
        raise AssertionError(f"{who}{name_of(task, z, int(idx[e]), t)}: {what}")

    if rew is not None:
        got, want = np.round(np.asarray(rew, np.float64) * 2).astype(np.int64), z["r_rewards_x2"][idx, t]
        if not np.array_equal(got, want):
            e, i = [int(v) for v in np.argwhere(got != want)[0]]
            fail(e, f"agent {i} reward {got[e, i] / 2}, reference {want[e, i] / 2}")
    if done is not None and not np.array_equal(np.asarray(done).astype(bool), z["r_done"][idx, t].astype(bool)):
        e = int(np.argwhere(np.asarray(done).astype(bool) != z["r_done"][idx, t].astype(bool))[0, 0])
        fail(e, f"done {bool(np.asarray(done)[e])}, reference {bool(z['r_done'][idx, t][e])}")


def check_same(task, z, idx, t, what, got, want, who="", *, name_of):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        e = _first_env(got, want)
        i = int(np.argwhere((got[e] != want[e]).reshape(got.shape[1], -1).any(-1))[0, 0]) if got.ndim > 1 else -1
        raise AssertionError(f"{who}{name_of(task, z, int(idx[e]), t)}: {what} of agent {i} differs from the oracle's")


# ------------------------------------------------------------------------------------------------------------------ the engine
def fixture_outputs(z, idx):
    """engine_run's `want` where no oracle exists (more than 64 agents): the fixture's own z["obs"] (n, 1 + T, N, L), rewards, done."""
    return [z["obs"][idx, 0]] + [(z["obs"][idx, t + 1], z["r_rewards_x2"][idx, t].astype(np.float32) / 2, z["r_done"][idx, t].astype(bool))
                                 for t in range(z["meta"]["steps"])]


def engine_run(task, z, idx, fused, who, kwargs, want, *, fields, name_of, library=None, after_step=None, **ctor):
    """The engine on the injected batch against the fixture (`fields`, rewards, done) and against `want` = [observation of the injected
    state, (observation, rewards, done) per step]: the oracle's, themselves checked against the fixture, or fixture_outputs.  A fused
    rollout hands back no state between its steps: there the three tapes at every step, the state behind the last one.
    `after_step(env, t)`: a pin's own check behind a per-step launch.  Returns the engine's rw_info."""
    import rware_amd      # (here: the generators import this module too, and run without the package on their path)
    same = lambda t, what, got, ref: check_same(task, z, idx, t, what, got, ref, who, name_of=name_of)      # noqa: E731
    state = lambda t, env, rew, term: check_state(task, z, idx, t, env.get_state(), env.shelf_xy(), rew, term, who,      # noqa: E731
                                                  fields=fields, name_of=name_of)
    env = rware_amd.WarehouseVecEnv(len(idx), autoreset_mode="disabled", library=library, **kwargs, **ctor)
    T = z["meta"]["steps"]
    try:
        unpack = env.unpack_obs if ctor.get("obs_format") == "packed" else (lambda o: o)
        same(0, "the observation of the injected state", unpack(inject(env, z, idx)), want[0])
        if fused:
            obs, rew, term = env.rollout(z["actions"][idx].astype(np.int32).transpose(1, 0, 2))
            for t in range(T):
                same(t, "observation (fused rollout)", unpack(obs[t]), want[t + 1][0])
                same(t, "reward (fused rollout)", rew[t], want[t + 1][1])
                same(t, "done (fused rollout)", term[t], want[t + 1][2].astype(bool))
            state(T - 1, env, rew[T - 1], term[T - 1])
        else:
            for t in range(T):
                obs, rew, term, trunc, _ = env.step(z["actions"][idx, t].astype(np.int32))
                state(t, env, rew, term)
                same(t, "observation", unpack(obs), want[t + 1][0])
                same(t, "reward", rew, want[t + 1][1])
                if after_step is not None:
                    after_step(env, t)
        return env.engines[0].info
    finally:
        env.close()
