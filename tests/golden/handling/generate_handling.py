"""Generates tests/golden/handling/*.npz by running the UNMODIFIED reference (found by oracle/ref_runner.py) on the constructed states of
tests/handling_scenarios.py.  Run:  python tests/golden/handling/generate_handling.py [task ...]

Per task and configuration of handling_scenarios.CONFIGS (the three reward types with `max_steps` / `max_inactivity_steps` set to
handling_scenarios.LIMITS, and TWO_STAGE with no limit) one reference `Warehouse` is reset once (seed in `meta`).  Every scenario
overwrites its objects the way the reference's own tests do — pins.inject_reference with `has_delivered`, `_cur_steps`,
`_cur_inactive_steps` and the PCG64 state — and takes T_STEPS steps under the pinned tie-break of oracle/ref_runner.py.

Stored per scenario: the injected state and the T x N actions; after every step the agents' x / y / dir / carry, every shelf's (x, y),
the queue, the generator words, the step's `choice` count and failed moves (ref_runner.ref_step_events) — none of which depends on the
configuration, which the generator checks — and per configuration `has_delivered`, rewards (x 2: TWO_STAGE halves stay integers), done
and the two counters.  No observations (they are compared engine <-> oracle), except where no oracle exists (more than 64 agents): there
the FLATTENED rows of the injected state and of every step are stored bit-packed (tests/wide_fixtures.pack_obs).

The generator refuses to write a task in which a family that its geometry admits yields no scenario, a scenario's census misses its claim,
or a class that the geometry admits is held by no scenario.
"""
import json
import os
import sys
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import handling_scenarios as hs  # noqa: E402
import pins  # noqa: E402
import ref_runner as rr  # noqa: E402
import rng_states as rs  # noqa: E402
import wide_fixtures as wf  # noqa: E402

SEED = 2027          # reset seed of every task
ROUND_SEED = 3       # turns the round of the id assignments
# five goals, two of them adjacent, a shelf cell straight behind the third: the whole story fits into six steps there
LAYOUT_5GOALS = "..gg...\n.xx.xx.\n.gx.xx.\n.xx.xx.\ng..g..."
_CUSTOM = dict(msg_bits=0, sensor_range=1, max_inactivity_steps=None, max_steps=500, reward_type=1)
# name -> (registered id or None, constructor overrides)
TASKS = {f"tiny-{n}ag": (f"rware-tiny-{n}ag-v2", {}) for n in (2, 4, 8, 9, 13, 16, 19)}
TASKS.update({
    "small-4ag": ("rware-small-4ag-v2", {}),
    "small-16ag": ("rware-small-16ag-v2", {}),
    "small-20ag": ("rware-small-16ag-v2", dict(n_agents=20)),                       # the LDS agent phases
    "29x28-10ag": (None, dict(_CUSTOM, shelf_columns=9, column_height=8, shelf_rows=3, n_agents=10, request_queue_size=10)),   # uint16 shelf layer
    "layout-5goals": (None, dict(_CUSTOM, shelf_columns=0, column_height=0, shelf_rows=0, n_agents=3, request_queue_size=3, layout=LAYOUT_5GOALS)),
    "tiny-65ag": (None, dict(_CUSTOM, shelf_columns=3, column_height=8, shelf_rows=1, n_agents=65, request_queue_size=20)),    # no oracle: observations stored
})
AGENT_FIELDS = ("agent_x", "agent_y", "agent_dir", "agent_carry")


def reference_env(name, c):
    wh = rr.load_reference()
    env_id, over = TASKS[name]
    rt, limited = hs.CONFIGS[c]
    kw = dict(over, reward_type=wh.RewardType(rt))
    kw.update(hs.LIMITS if limited else dict(max_steps=None, max_inactivity_steps=None))
    env = rr.make_reference_env(env_id, **kw)
    env.reset(seed=SEED)
    return env


def shape_of(env):
    H, W = env.grid_size
    return dict(H=int(H), W=int(W), N=env.n_agents, S=len(env.shelfs), Q=env.request_queue_size, goals=[(int(x), int(y)) for x, y in env.goals],
                highways=np.asarray(env.highways).astype(np.uint8), shelf_xy=np.array([[s.x, s.y] for s in env.shelfs], np.int32),
                queue=np.array([s.id for s in env.request_queue], np.int32), rng0=rr.rng_state_tuple(env))


def state_of(env):
    snap = rr.snapshot(env)
    snap["shelf_xy"] = np.array([[s.x, s.y] for s in env.shelfs], np.int32)
    return snap


def small(a):
    a = np.asarray(a)
    return a.astype(np.int8 if a.max(initial=0) < 128 and a.min(initial=0) >= -128 else np.int16 if a.max(initial=0) < 32768 else np.int32)


def record_task(name, out_dir=HERE):
    envs = [reference_env(name, c) for c in range(len(hs.CONFIGS))]
    shape = shape_of(envs[0])
    N, S, Q, T, C = shape["N"], shape["S"], shape["Q"], hs.T_STEPS, len(hs.CONFIGS)
    scen = hs.build_scenarios(shape, seed=ROUND_SEED)
    n = len(scen)
    families, classes = hs.admitted(shape)
    missing = families - {sc["family"] for sc in scen}
    assert not missing, f"{name}: no scenario of the admitted families {sorted(missing)}"
    rec = {f"r_{k}": np.zeros((n, T, N), np.int32) for k in AGENT_FIELDS}
    rec.update(r_shelf_xy=np.zeros((n, T, S, 2), np.int32), r_queue=np.zeros((n, T, Q), np.int32), r_rng=np.zeros((n, T, 6), np.uint64),
               r_choice=np.zeros((n, T), np.int32), r_failed=np.zeros((n, T), np.int32),
               r_agent_delivered=np.zeros((n, C, T, N), np.int32), r_rewards_x2=np.zeros((n, C, T, N), np.int32), r_done=np.zeros((n, C, T), np.int32),
               r_steps=np.zeros((n, C, T), np.int32), r_inactive=np.zeros((n, C, T), np.int32))
    wide = N > 64
    obs = np.zeros((n, T + 1, N, envs[0].observation_space[0].shape[0]), np.float32) if wide else None
    census = [Counter() for _ in range(C)]
    for k, sc in enumerate(scen):
        for c, env in enumerate(envs):
            pins.inject_reference(env, sc, rs.numpy_state(sc["rng"]), counters=True)
            sh = hs.config_shape(shape, c)
            before, by_step = state_of(env), []
            if wide and c == 0:
                obs[k, 0] = rr.obs_array(tuple(env._make_obs(a) for a in env.agents))
            for t in range(T):
                (o, rew, done, _, _), choice, failed = rr.ref_step_events(env, [int(a) for a in sc["actions"][t]])
                after = state_of(env)
                by_step.append(hs.handling_census(before, sc["actions"][t], after, choice, sh))
                assert hs.count_deliveries(before, sc["actions"][t], rew, sh) == choice, (name, sc["variant"], c, t)
                shared = dict({f: after[f] for f in AGENT_FIELDS}, shelf_xy=after["shelf_xy"], queue=after["queue"], rng=after["rng"], choice=choice, failed=failed)
                for f, v in shared.items():
                    if c == 0:
                        rec["r_" + f][k, t] = v
                    else:
                        assert np.array_equal(rec["r_" + f][k, t], v), f"{name}, {sc['variant']}, step {t}: {f} depends on the configuration"
                rec["r_agent_delivered"][k, c, t], rec["r_rewards_x2"][k, c, t] = after["agent_delivered"], np.round(np.asarray(rew, np.float64) * 2)
                rec["r_done"][k, c, t], rec["r_steps"][k, c, t], rec["r_inactive"][k, c, t] = int(done), after["steps"], after["inactive"]
                if wide and c == 0:
                    obs[k, t + 1] = rr.obs_array(o)
                before = after
            assert hs.claim_holds(by_step, sc["claim"], hs.CONFIGS[c][1]), \
                f"{name}, scenario {k} ({sc['family']} / {sc['variant']}, ids {sc['ids']}), configuration {c}: claims {sc['claim']}, the census found {[dict(b) for b in by_step]}"
            for b in by_step:
                census[c].update(b)
    held = set().union(*census)
    assert classes <= held, f"{name}: no scenario holds {sorted(classes - held)}"
    out = {k: (v if k == "r_rng" else small(v)) for k, v in rec.items()}
    for key in AGENT_FIELDS + ("agent_delivered", "shelf_xy", "queue", "actions", "steps", "inactive"):
        out[key] = small(np.stack([sc[key] for sc in scen]))
    out["rng"] = np.stack([sc["rng"] for sc in scen]).astype(np.uint64)
    fam = [sc["family"] for sc in scen]
    meta = {
        "name": name, "env_id": TASKS[name][0], "overrides": TASKS[name][1], "H": shape["H"], "W": shape["W"], "N": N, "S": S, "Q": Q, "goals": shape["goals"],
        "seed": SEED, "round_seed": ROUND_SEED, "n": n, "steps": T, "configs": [list(c) for c in hs.CONFIGS], "limits": hs.LIMITS,
        "tie_break": "lowest_agent_id", "gymnasium": "standin" if rr.using_standin_gymnasium() else "real",
        "reference": "semitable/robotic-warehouse (rware 2.0.0)",
        "families": {f: fam.count(f) for f in hs.FAMILIES}, "id_assignments": {a: sum(sc["ids"] == a for sc in scen) for a in hs.ID_ASSIGNMENTS},
        "census": [dict(sorted(c.items())) for c in census],
    }
    extra = {}
    if wide:
        meta["obs_shape"] = [int(obs.shape[-1])]
        extra = wf.pack_obs(obs, True, 3)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, meta=json.dumps(meta), highways=shape["highways"], rng0=shape["rng0"], queue0=small(shape["queue"]),
                        family=np.array([hs.FAMILIES.index(f) for f in fam], np.int8),
                        ids=np.array([hs.ID_ASSIGNMENTS.index(sc["ids"]) for sc in scen], np.int8),
                        variant=np.array([sc["variant"] for sc in scen]), claim=np.array([sc["claim"] for sc in scen]), **out, **extra)
    print(f"{name}: N={N} S={S} scenarios={n} {meta['families']} -> {os.path.getsize(path) / 1024:.0f} KiB")
    return path


def trace_shape(kw, grid_shape):
    """The census' `shape` of a golden trace, from its constructor arguments (`meta["kwargs"]`)."""
    from rware_oracle import layout_from_params, layout_from_str
    hw, goals = layout_from_str(kw["layout"]) if kw.get("layout") else layout_from_params(kw["shelf_columns"], kw["shelf_rows"], kw["column_height"])
    assert hw.shape == tuple(grid_shape)
    return dict(H=hw.shape[0], W=hw.shape[1], N=kw["n_agents"], Q=kw["request_queue_size"], goals=goals, highways=hw, reward_type=int(kw["reward_type"]),
                max_steps=kw.get("max_steps"), max_inactivity_steps=kw.get("max_inactivity_steps"))


def trace_census(meta, z):
    """The census over every env-step of one golden trace (tests/golden/*.npz, tests/golden/wide/*.npz; reset steps left out): the
    delivery count of a step from its rewards (handling_scenarios.count_deliveries)."""
    shape = trace_shape(meta["kwargs"], z["grid"].shape[-2:])
    fields = ("agent_x", "agent_y", "agent_dir", "agent_carry", "agent_delivered", "queue", "steps", "inactive")
    z = {k: z[k] for k in [p + f for f in fields + ("grid",) for p in ("init_", "")] + ["actions", "rewards", "was_reset"]}   # (an .npz unpacks per access)
    total = Counter()
    T, E = z["actions"].shape[:2]
    for e in range(E):
        before = dict({f: z["init_" + f][e] for f in fields}, shelf_layer=z["init_grid"][e, 1])
        for t in range(T):
            after = dict({f: z[f][t, e] for f in fields}, shelf_layer=z["grid"][t, e, 1])
            if not z["was_reset"][t, e]:
                a = z["actions"][t, e]
                a = a[:, 0] if a.ndim == 2 else a
                d = hs.count_deliveries(before, a, z["rewards"][t, e], shape)
                total.update(hs.handling_census(before, a, after, d, shape))
                total["env_steps"] += 1
            before = after
    return total


def golden_traces():
    """[(name, meta, fields)] of every committed trace of the reference: tests/golden/*.npz and the traces of tests/golden/wide/."""
    import golden_util as gu
    out = [(name,) + tuple(gu.load_fixture(name)) for name in gu.fixture_names()]
    return out + [("wide/" + name,) + tuple(wf.load_trace(name)) for name in wf.TRACES + wf.SCRIPTED]


def record_trace_census(out_dir=HERE):
    """trace_census.json: what random and scripted play reached — per trace and in all — for the test that asks the fixtures to hold at
    least that."""
    per = {name: dict(sorted(trace_census(meta, z).items())) for name, meta, z in golden_traces()}
    total = Counter()
    for c in per.values():
        total.update(c)
    path = os.path.join(out_dir, "trace_census.json")
    with open(path, "w") as f:
        json.dump({"total": dict(sorted(total.items())), "traces": per}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"trace census over {len(per)} traces: {dict(sorted(total.items()))}")
    return path


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for task in TASKS:
        if not only or task in only:
            record_task(task)
    if not only or "trace_census" in only:
        record_trace_census()
