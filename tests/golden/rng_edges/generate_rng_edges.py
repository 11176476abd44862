"""Generates tests/golden/rng_edges/*.npz by running the UNMODIFIED reference (found by oracle/ref_runner.py) on the constructed
generator states of tests/rng_states.py.  Run:  python tests/golden/rng_edges/generate_rng_edges.py
The task ids of rng_states.TASKS end in -v2: that is what the reference registers; this package's rware-*-v1 ids name the same shapes.

Per task (rng_states.TASKS) one reference `Warehouse` is reset once (seed in `meta`).
  Reset scenarios (rs_*): the constructed state goes into `env.np_random`, then `reset()` with no seed.  Stored: the state before
  (rs_rng0), and after it agent_x / agent_y / agent_dir, the queue and the six state words (rs_r_*).
  Delivery scenarios (dl_*): requested shelves are put onto goal cells by tests/pins.inject_reference (objects overwritten,
  `_recalc_grid()`), the constructed state goes into `env.np_random`, one all-NOOP step follows.  Stored: the injected state (agents,
  every shelf's (x, y), queue, state words) and after the step the queue, rewards (x 2, so TWO_STAGE halves stay integers), done,
  agent_delivered and the state words (dl_r_*).
`meta` holds the scenario names, the claim of each and the counts; no observations (they are compared engine <-> oracle).
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
import pins  # noqa: E402
import ref_runner as rr  # noqa: E402
import rng_states as rs  # noqa: E402

SEED = 2025          # reset seed of every task; its increment is the one every constructed state of the task carries


def delivery_state(sc, H, W, N, highways, goals):
    """The arrays one delivery scenario injects: agents on the first free cells in row-major order that are no goal (direction UP,
    nothing carried), shelves at home except the delivered ones, which sit on their goal cells; `who` puts an agent there."""
    free = [(x, y) for y in range(H) for x in range(W) if (x, y) not in goals][:N]
    ax, ay = np.array([c[0] for c in free], np.int32), np.array([c[1] for c in free], np.int32)
    carry = np.zeros(N, np.int32)
    sxy = rs.shelf_home(highways)
    first = True
    for g, sid in enumerate(sc.on_goal):
        if not sid:
            continue
        sxy[sid - 1] = goals[g]
        if first and sc.who != "nobody":
            i = 0 if sc.who == "agent_0_carrying" else max(N - 2, 0)
            ax[i], ay[i] = goals[g]
            carry[i] = sid if sc.who == "agent_0_carrying" else 0
        first = False
    return dict(agent_x=ax, agent_y=ay, agent_dir=np.zeros(N, np.int32), agent_carry=carry, shelf_xy=sxy, queue=np.array(sc.queue, np.int32))


def record_task(name, out_dir=HERE):
    wh = rr.load_reference()
    env_id, over = rs.TASKS[name]
    kw = dict(over)
    if "reward_type" in kw:
        kw["reward_type"] = wh.RewardType(kw["reward_type"])
    env = rr.make_reference_env(env_id, **kw)
    env.reset(seed=SEED)
    H, W = env.grid_size
    N, S, Q = env.n_agents, len(env.shelfs), env.request_queue_size
    goals = [(int(x), int(y)) for x, y in env.goals]
    highways = np.asarray(env.highways)
    assert np.array_equal(rs.shelf_home(highways), np.array([[s.x, s.y] for s in env.shelfs]))
    inc = env.np_random.bit_generator.state["state"]["inc"]

    resets = rs.reset_scenarios(H * W, N, S, Q, inc)
    rec = dict(rs_rng0=np.stack([sc.state for sc in resets]), rs_r_rng=np.zeros((len(resets), 6), np.uint64),
               rs_r_queue=np.zeros((len(resets), Q), np.int16))
    for f in ("agent_x", "agent_y", "agent_dir"):
        rec["rs_r_" + f] = np.zeros((len(resets), N), np.int8)
    for k, sc in enumerate(resets):
        env.np_random.bit_generator.state = rs.numpy_state(sc.state)
        env.reset()
        snap = rr.snapshot(env)
        for f in ("agent_x", "agent_y", "agent_dir"):
            rec["rs_r_" + f][k] = snap[f]
        rec["rs_r_queue"][k], rec["rs_r_rng"][k] = snap["queue"], snap["rng"]

    deliveries = rs.delivery_scenarios(S, Q, N, len(goals), inc)
    nd = len(deliveries)
    rec.update(dl_rng0=np.stack([sc.state for sc in deliveries]), dl_r_rng=np.zeros((nd, 6), np.uint64),
               dl_on_goal=np.array([sc.on_goal for sc in deliveries], np.int16),
               dl_r_queue=np.zeros((nd, Q), np.int16), dl_r_rewards_x2=np.zeros((nd, N), np.int8), dl_r_done=np.zeros(nd, np.int8),
               dl_r_agent_delivered=np.zeros((nd, N), np.int8))
    states = [delivery_state(sc, H, W, N, highways, goals) for sc in deliveries]
    for f, dt in (("agent_x", np.int8), ("agent_y", np.int8), ("agent_dir", np.int8), ("agent_carry", np.int16), ("shelf_xy", np.int8), ("queue", np.int16)):
        rec["dl_" + f] = np.stack([st[f] for st in states]).astype(dt)
    for k, (sc, st) in enumerate(zip(deliveries, states)):
        env.reset(seed=SEED)        # (fresh Shelf / Agent objects: a delivery scenario starts from the same env every time)
        pins.inject_reference(env, st, rs.numpy_state(sc.state))
        _, rew, done, _, _ = rr.ref_step(env, [0] * N)
        snap = rr.snapshot(env)
        rec["dl_r_queue"][k], rec["dl_r_rng"][k] = snap["queue"], snap["rng"]
        rec["dl_r_rewards_x2"][k] = np.round(np.asarray(rew, np.float64) * 2)
        rec["dl_r_done"][k], rec["dl_r_agent_delivered"][k] = int(done), snap["agent_delivered"]
    meta = {
        "name": name, "env_id": env_id, "overrides": over, "H": int(H), "W": int(W), "N": int(N), "S": int(S), "Q": int(Q),
        "goals": goals, "seed": SEED, "reward_type": int(env.reward_type.value),
        "gymnasium": "standin" if rr.using_standin_gymnasium() else "real", "reference": "semitable/robotic-warehouse (rware 2.0.0)",
        "n_reset": len(resets), "n_delivery": nd,
        "reset_names": [sc.name for sc in resets], "reset_claims": [sc.claim for sc in resets],
        "delivery_names": [sc.name for sc in deliveries], "delivery_claims": [sc.claim for sc in deliveries],
        "delivery_who": {w: sum(sc.who == w for sc in deliveries) for w in rs.WHO},
        "deliveries_with_rejection": sum(any((d[0] or 0) > 0 for d in sc.draws) for sc in deliveries),
    }
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **rec)
    print(f"{name}: N={N} S={S} Q={Q} reset scenarios={len(resets)} delivery scenarios={nd} -> {os.path.getsize(path) / 1024:.0f} KiB")
    return path


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for task in rs.TASKS:
        if not only or task in only:
            record_task(task)
