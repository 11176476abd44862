"""Generates tests/golden/observations/*.npz by running the UNMODIFIED reference (/root/reference/rware) in the build container on the
constructed observation scenarios of tests/observation_scenarios.py.  Run:  python tests/golden/observations/generate_observations.py

Per task one reference `Warehouse` is reset once (seed in `meta`); every scenario is injected the way
tests/pins.inject_reference does it (objects overwritten, counters 0, the PCG64 state of the reset,
`_recalc_grid()`; messages cleared), then:

  observation 0    `_make_obs` of every agent on the injected state
  step 0           all NOOP (the goals family: its deliveries), carrying each agent's message bits where msg_bits > 0
  step 1           seeded mixed actions

under the pinned tie-break of oracle/ref_runner.py.  Stored per scenario: the injected state, the 2 x N actions, the three
observations of every agent in the task's observation type (IMAGE_DICT: the features too), and after each step the agents, every
shelf's (x, y), the queue, rewards (x 2), done and the PCG64 words.  0/1 observation elements are stored bit-packed (np.packbits
over the last axis); the two coordinates of a FLATTENED row stay float32.  A scenario of the goals family carries its reward type.

`meta` holds the census of the injected states (tests/observation_scenarios.window_census), the family counts and the random-play
floor: how many census classes random play (`floor_play` envs x steps) reaches on the C oracle, beside how many the fixture holds.
"""
import json
import os
import sys
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import observation_scenarios as osc  # noqa: E402
import pins  # noqa: E402
import ref_runner as rr  # noqa: E402

SEED = 2025          # reset seed of every task
SAMPLE_SEED = 11     # seed of the scenarios' queues, parked agents and step-1 actions


def floor_play(n_agents, sensor_range, shelf_rows):
    """envs x steps of the random-play floor, by the nearest row of the table the measurement was first made with: 7 x 400 on the
    2-agent tasks, 64 x 100 on the small warehouse, 16 x 200 on sensor ranges 2 .. 5 and on everything else."""
    if sensor_range >= 2:
        return 16, 200
    return (7, 400) if n_agents == 2 else (64, 100) if shelf_rows == 2 else (16, 200)


LAYOUTS = {
    "1goal": """
        ......
        .xx.x.
        .xx.x.
        ......
        ..g...""",
    # one goal on the top row, one off the bottom row
    "3goals": """
        ..g...
        .xx.xx
        g.....
        .xx.xx
        ...g..""",
    "5goals": """
        .g..g..
        .xx.xx.
        g.....g
        .xx.xx.
        ...g...""",
    "16goals": """
        gggggggg
        .xx..xx.
        .xx..xx.
        ........
        .xx..xx.
        gggggggg""",
}


def _layout_kwargs(name, image):
    kw = {"shelf_columns": 0, "column_height": 0, "shelf_rows": 0, "n_agents": 3, "msg_bits": 0, "sensor_range": 1, "request_queue_size": 3,
          "max_inactivity_steps": None, "max_steps": 200, "reward_type": 1, "layout": "\n".join(l.strip() for l in LAYOUTS[name].strip().split("\n"))}
    if image:
        kw.update(observation_type=2, image_observation_layers=[0, 1, 2, 5, 6])
    return kw


_SQUARE = {"shelf_columns": 3, "column_height": 3, "shelf_rows": 2, "n_agents": 4, "msg_bits": 0, "sensor_range": 1, "request_queue_size": 4,
           "max_inactivity_steps": None, "max_steps": 500, "reward_type": 1, "observation_type": 2, "image_observation_layers": [0, 1, 2, 3, 4, 5, 6]}
_BIG = {"shelf_columns": 9, "column_height": 8, "shelf_rows": 3, "n_agents": 10, "msg_bits": 0, "sensor_range": 1, "request_queue_size": 10,
        "max_inactivity_steps": None, "max_steps": 500, "reward_type": 1}
# name -> (registered id or None, extra constructor arguments)
TASKS = {
    "tiny-4ag": ("rware-tiny-4ag-v2", {}),
    "tiny-9ag": ("rware-tiny-9ag-v2", {}),
    "tiny-19ag": ("rware-tiny-19ag-v2", {}),
    "tiny-3ag-sr2": ("rware-tiny-3ag-v2", {"sensor_range": 2}),
    "tiny-3ag-sr3": ("rware-tiny-3ag-v2", {"sensor_range": 3}),
    "tiny-3ag-sr4": ("rware-tiny-3ag-v2", {"sensor_range": 4}),
    "tiny-2ag-sr5": ("rware-tiny-2ag-v2", {"sensor_range": 5}),
    "tiny-3ag-msg1": ("rware-tiny-3ag-v2", {"msg_bits": 1}),
    "tiny-3ag-msg2": ("rware-tiny-3ag-v2", {"msg_bits": 2}),
    "tiny-3ag-msg3-sr2": ("rware-tiny-3ag-v2", {"msg_bits": 3, "sensor_range": 2}),
    "small-3ag-normcoord": ("rware-small-3ag-v2", {"normalised_coordinates": True}),
    "29x28-10ag": (None, _BIG),
    "img-tiny-3ag-directional-sr2": ("rware-tiny-3ag-v2", {"observation_type": 2, "sensor_range": 2}),
    "img-tiny-3ag-northup": ("rware-tiny-3ag-v2", {"observation_type": 2, "image_observation_directional": False}),
    "img-square-4ag-all7": (None, _SQUARE),
    "imgdict-tiny-2ag": ("rware-tiny-2ag-v2", {"observation_type": 3}),
}
for _n in LAYOUTS:
    TASKS[f"layout-{_n}"] = (None, _layout_kwargs(_n, False))
    TASKS[f"img-layout-{_n}"] = (None, _layout_kwargs(_n, True))


def reference_env(env_id, extra):
    wh = rr.load_reference()
    kw = rr.registry_kwargs(env_id) if env_id else {}
    kw.update(extra)
    kw["reward_type"] = wh.RewardType(int(getattr(kw["reward_type"], "value", kw["reward_type"])))
    kw["observation_type"] = wh.ObservationType(int(kw.get("observation_type", 1)))
    if "image_observation_layers" in kw:
        kw["image_observation_layers"] = [wh.ImageLayer(int(l)) for l in kw["image_observation_layers"]]
    return wh.Warehouse(**kw)


def shape_of(env, goals_family=False):
    """The task's shape, read off a reference env after reset()."""
    H, W = env.grid_size
    sh = osc.make_shape(np.asarray(env.highways), env.goals, env.n_agents, env.request_queue_size, env.sensor_range, env.msg_bits,
                        goals_family=goals_family)
    assert (sh["H"], sh["W"]) == (H, W) and np.array_equal(sh["home"], [[s.x, s.y] for s in env.shelfs])
    return sh


def inject(env, sc, rng_state):
    """pins.inject_reference, plus what the other pins have no need for: messages cleared, the scenario's reward type."""
    wh = rr.load_reference()
    pins.inject_reference(env, sc, rng_state)
    for ag in env.agents:
        ag.message[:] = 0
    if sc.get("reward_type") is not None:
        env.reward_type = wh.RewardType(int(sc["reward_type"]))


def observe(env):
    """(observation, features or None) of every agent, as arrays."""
    o = tuple(env._make_obs(a) for a in env.agents)
    return arrays_of(o)


def arrays_of(o):
    if isinstance(o[0], dict):
        return np.stack([a["image"] for a in o]).astype(np.float32), np.stack([a["features"] for a in o]).astype(np.float32)
    return rr.obs_array(o), None


def pack_observations(obs, flattened):
    """float32 observations -> the arrays stored: FLATTENED (…, L): the coordinates as float32 + the rest as bits; images: bits, or
    bytes where a layer holds more than 0 / 1 (AGENT_DIRECTION)."""
    if flattened:
        rest = obs[..., 2:]
        assert np.isin(rest, (0.0, 1.0)).all()
        return {"obs_xy": obs[..., :2].astype(np.float32), "obs_bits": np.packbits(rest.astype(np.uint8), axis=-1)}
    flat = obs.reshape(obs.shape[:3] + (-1,))
    assert np.array_equal(flat, flat.astype(np.uint8))
    if flat.max() <= 1:
        return {"img_bits": np.packbits(flat.astype(np.uint8), axis=-1)}
    return {"img_u8": flat.astype(np.uint8)}


def record_task(name, out_dir=HERE):
    from rware_oracle import OracleVecEnv
    env_id, extra = TASKS[name]
    env = reference_env(env_id, extra)
    default_reward = int(env.reward_type.value)
    env.reset(seed=SEED)
    sh = shape_of(env, goals_family="layout" in extra)
    N, S, Q, M = sh["N"], sh["S"], sh["Q"], sh["M"]
    rng_state = env.np_random.bit_generator.state
    rng0 = rr.rng_state_tuple(env)
    scen = osc.build_scenarios(sh, seed=SAMPLE_SEED)
    n, T = len(scen), osc.T_STEPS
    keys = ("agent_x", "agent_y", "agent_dir", "agent_carry", "agent_delivered")
    rec = {f"r_{k}": np.zeros((n, T, N), np.int16) for k in keys}
    rec.update(r_shelf_xy=np.zeros((n, T, S, 2), np.int16), r_queue=np.zeros((n, T, Q), np.int16), r_rewards_x2=np.zeros((n, T, N), np.int16),
               r_done=np.zeros((n, T), np.int16), r_deliveries=np.zeros((n, T), np.int16))
    r_rng = np.zeros((n, T, 6), np.uint64)
    if M:
        rec["r_agent_msg"] = np.zeros((n, T, N), np.int16)
    obs, feats = [], []
    census = Counter()
    for k, sc in enumerate(scen):
        inject(env, sc, rng_state)
        census.update(osc.window_census(sc, sh, osc.msg_values(sc["actions"][0])))
        o3, f3 = [], []
        o, f = observe(env)
        o3.append(o)
        f3.append(f)
        for t in range(T):
            a = sc["actions"][t]
            acts = [[int(v) for v in row] for row in a] if M else [int(v) for v in a[:, 0]]
            (o, rew, done, _, _), delivered, _ = rr.ref_step_events(env, acts)
            o, f = arrays_of(o)
            o3.append(o)
            f3.append(f)
            snap = rr.snapshot(env)
            for key in keys:
                rec[f"r_{key}"][k, t] = snap[key]
            rec["r_shelf_xy"][k, t] = [[s.x, s.y] for s in env.shelfs]
            rec["r_queue"][k, t] = snap["queue"]
            rec["r_rewards_x2"][k, t] = np.round(np.asarray(rew, np.float64) * 2)
            rec["r_done"][k, t] = int(done)
            rec["r_deliveries"][k, t] = delivered
            r_rng[k, t] = snap["rng"]
            if M:
                rec["r_agent_msg"][k, t] = snap["agent_msg"]
        obs.append(np.stack(o3))
        if f3[0] is not None:
            feats.append(np.stack(f3))
    small = lambda a: a.astype(np.int8 if a.max(initial=0) < 128 else np.int16)  # noqa: E731
    out = {k: small(v) for k, v in rec.items()}
    for key in ("agent_x", "agent_y", "agent_dir", "agent_carry", "shelf_xy", "queue", "actions"):
        out[key] = small(np.stack([sc[key] for sc in scen]))
    obs = np.stack(obs)
    obs_type = int(extra.get("observation_type", 1))
    out.update(pack_observations(obs, obs.ndim == 4))
    if feats:
        out["feat_u8"] = np.stack(feats).astype(np.uint8)
        assert np.array_equal(out["feat_u8"], np.stack(feats))
    # the random-play floor, on the C oracle: what 16 envs x 200 steps reach of the classes the fixture holds
    okw = dict(rr.registry_kwargs(env_id) if env_id else {}, **extra)
    okw["reward_type"] = default_reward
    FLOOR_ENVS, FLOOR_STEPS = floor_play(N, sh["R"], int(okw.get("shelf_rows", 0)))
    played = osc.random_play_classes(OracleVecEnv(FLOOR_ENVS, **okw), sh, FLOOR_STEPS)
    fam = [sc["family"] for sc in scen]
    meta = {
        "name": name, "env_id": env_id, "kwargs": extra, "H": sh["H"], "W": sh["W"], "N": N, "S": S, "Q": Q, "R": sh["R"], "M": M,
        "obs_shape": list(obs.shape[2:]), "observation_type": obs_type,
        "seed": SEED, "sample_seed": SAMPLE_SEED, "n": n, "steps": T, "tie_break": "lowest_agent_id",
        "gymnasium": "standin" if rr.using_standin_gymnasium() else "real", "reference": "semitable/robotic-warehouse (rware 2.0.0)",
        "families": {f: fam.count(f) for f in osc.FAMILIES if fam.count(f)},
        "census": {osc.census_key(c): v for c, v in sorted(census.items(), key=lambda cv: osc.census_key(cv[0]))},
        "deliveries": int(rec["r_deliveries"].sum()),
        "floor": {"envs": FLOOR_ENVS, "steps": FLOOR_STEPS, "classes_random_play": len(set(played) & set(census)),
                  "classes_fixture": len(census), "classes_only_random_play": len(set(played) - set(census))},
    }
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, meta=json.dumps(meta), rng0=rng0, r_rng=r_rng,
                        family=np.array([osc.FAMILIES.index(f) for f in fam], np.int8), ids=np.array([sc["ids"] for sc in scen], np.int8),
                        reward_type=np.array([default_reward if sc["reward_type"] is None else sc["reward_type"] for sc in scen], np.int8),
                        variant=np.array([sc["variant"] for sc in scen]), **out)
    print(f"{name}: N={N} scenarios={n} {meta['families']} classes {len(census)} (random play reaches {meta['floor']['classes_random_play']}, "
          f"+{meta['floor']['classes_only_random_play']} others) deliveries {meta['deliveries']} -> {os.path.getsize(path) / 1024:.0f} KiB")
    return path


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for task in TASKS:
        if not only or task in only:
            record_task(task)
