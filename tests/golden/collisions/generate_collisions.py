"""Generates tests/golden/collisions/*.npz by running the UNMODIFIED reference (/root/reference/rware) in the build container
on the constructed collision scenarios of tests/collision_scenarios.py.  Run:  python tests/golden/collisions/generate_collisions.py

Per task one reference `Warehouse` is reset once (seed in `meta`); every scenario overwrites its objects the way the reference's
own tests do (agents' x / y / dir / carrying_shelf, shelves' x / y, request_queue, counters 0, the PCG64 state of the reset),
calls `_recalc_grid()`, and takes 4 steps under the pinned tie-break of oracle/ref_runner.py (lowest agent id among equal-depth
predecessors).  Stored per scenario: the injected state, the 4 x N actions, and after each step the agents, every shelf's (x, y),
the queue, rewards (x 2, so TWO_STAGE halves stay integers), done, and the reference's `req_action` (what it turned each request
into: the failed-move count of the event counters follows from it).  No observations: they are compared engine <-> oracle.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import collision_scenarios as cs  # noqa: E402
import pins  # noqa: E402
import ref_runner as rr  # noqa: E402

SEED = 2024          # reset seed of every task
SAMPLE_SEED = 7      # seed of the id permutations and of the thinning sample
# name -> (registered id, cap on the number of scenarios)
TASKS = {f"tiny-{n}ag": (f"rware-tiny-{n}ag-v2", cap) for n, cap in
         [(2, 400), (3, 400), (4, 600), (5, 600), (6, 900), (7, 900), (8, 900), (9, 1200), (12, 1200), (13, 1200), (16, 1200), (17, 1200), (19, 1200)]}
TASKS["small-4ag"] = ("rware-small-4ag-v2", 600)
TASKS["small-16ag"] = ("rware-small-16ag-v2", 1200)


def record_task(name, out_dir=HERE):
    env_id, cap = TASKS[name]
    env = rr.make_reference_env(env_id)
    env.reset(seed=SEED)
    H, W = env.grid_size
    N, S = env.n_agents, len(env.shelfs)
    base = dict(H=H, W=W, N=N,
                shelf_xy=np.array([[s.x, s.y] for s in env.shelfs], np.int32),
                queue=np.array([s.id for s in env.request_queue], np.int32))
    rng_state = env.np_random.bit_generator.state
    rng0 = rr.rng_state_tuple(env)
    scen = cs.build_scenarios(base, seed=SAMPLE_SEED, cap=cap)
    n = len(scen)
    keys = ("agent_x", "agent_y", "agent_dir", "agent_carry", "agent_delivered")
    rec = {f"r_{k}": np.zeros((n, cs.T_STEPS, N), np.int16) for k in keys}
    rec.update(r_shelf_xy=np.zeros((n, cs.T_STEPS, S, 2), np.int16), r_queue=np.zeros((n, cs.T_STEPS, len(base["queue"])), np.int16),
               r_rewards_x2=np.zeros((n, cs.T_STEPS, N), np.int16), r_done=np.zeros((n, cs.T_STEPS), np.int16),
               r_req_action=np.zeros((n, cs.T_STEPS, N), np.int16))
    classes = {}
    for k, sc in enumerate(scen):
        pins.inject_reference(env, sc, rng_state)
        cen = cs.census(sc, sc["actions"][0], H, W, cs.shelf_layer_from_xy(sc["shelf_xy"], H, W))
        for c, v in cen.items():
            classes[c] = classes.get(c, 0) + v
        for t in range(cs.T_STEPS):
            _, rew, done, _, _ = rr.ref_step(env, [int(a) for a in sc["actions"][t]])
            snap = rr.snapshot(env)
            for key in keys:
                rec[f"r_{key}"][k, t] = snap[key]
            rec["r_shelf_xy"][k, t] = [[s.x, s.y] for s in env.shelfs]
            rec["r_queue"][k, t] = snap["queue"]
            rec["r_rewards_x2"][k, t] = np.round(np.asarray(rew, np.float64) * 2)
            rec["r_done"][k, t] = int(done)
            rec["r_req_action"][k, t] = [ag.req_action.value for ag in env.agents]
    small = lambda a: a.astype(np.int8 if a.max(initial=0) < 128 else np.int16)  # noqa: E731
    out = {k: small(v) for k, v in rec.items()}
    for key in keys + ("shelf_xy", "queue", "actions"):
        out[key] = small(np.stack([sc[key] for sc in scen]))
    fam = [sc["family"] for sc in scen]
    meta = {
        "name": name, "env_id": env_id, "H": int(H), "W": int(W), "N": int(N), "seed": SEED, "sample_seed": SAMPLE_SEED, "cap": cap, "n": n, "steps": cs.T_STEPS,
        "tie_break": "lowest_agent_id", "gymnasium": "standin" if rr.using_standin_gymnasium() else "real",
        "reference": "semitable/robotic-warehouse (rware 2.0.0)",
        "families": {f: fam.count(f) for f in cs.FAMILIES}, "id_assignments": {a: sum(sc["ids"] == a for sc in scen) for a in cs.ID_ASSIGNMENTS},
        "census_step0": dict(sorted(classes.items())),
    }
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, meta=json.dumps(meta), rng0=rng0,
                        family=np.array([cs.FAMILIES.index(f) for f in fam], np.int8),
                        ids=np.array([cs.ID_ASSIGNMENTS.index(sc["ids"]) for sc in scen], np.int8),
                        variant=np.array([sc["variant"] for sc in scen]), claim=np.array([sc["claim"] for sc in scen]), **out)
    print(f"{name}: N={N} scenarios={n} {meta['families']} -> {os.path.getsize(path) / 1024:.0f} KiB")
    return path


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for task in TASKS:
        if not only or task in only:
            record_task(task)
