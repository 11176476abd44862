"""Generates tests/golden/wide/*.npz by running the UNMODIFIED reference (oracle/ref_runner.load_reference) on warehouses of 65 .. 127
agents.  Run:  python tests/golden/wide/generate_wide.py [name ...]

The C oracle stops at 64 agents, so engines with more are checked against the reference itself.  Two kinds of fixture:

  random traces (TRACES)   the field layout of tests/golden/generate_golden.py — so golden_util.replay takes them — with the
      observations stored bit-packed as tests/golden/observations/generate_observations.py does (tests/wide_fixtures.py packs and
      unpacks).  E = 2 envs (env e seeded seed + e), NEXT_STEP autoreset, FORWARD-heavy seeded actions p = [.05, .7, .1, .1, .05];
      `max_steps` is small enough that every trace resets at least twice.  Every trace must hold a committed chain of movers with
      members on both sides of agent index 64 (wide_fixtures.trace_straddles): the generator refuses to write one that does not.
  collisions-straddle      constructed states on the 20 x 10 warehouse with 127 agents, built with tests/collision_scenarios.py
      (_Proto / _emit under explicit agent ids) and recorded as tests/golden/collisions/generate_collisions.py does — plus the
      observations, since no oracle can supply them.  Their structures cross the slot boundary (index 63 | 64); agents are named by
      their 0-based index, except "id 127", the last agent (index 126): loaded, its agent-layer byte is 0xFF.
          chain-62-65       a draining chain through agents 62, 63, 64, 65
          cycle-62-65       the rotation 62 -> 63 -> 64 -> 65 -> 62 (the shortest cycle a grid has: it is bipartite, so three
                            agents cannot rotate; the rule "three or more commit" is met by four)
          swap-0-64         a refused 2-swap of agents 0 and 64
          tie-3-70          a cell contested at equal depth by agents 3 and 70: 3 wins
          deeper-70-3       ... by a chain headed by agent 70 (71 behind it) against the lone agent 3: 70 wins
          blocked-64        agents 63 and 65 behind agent 64, who stays
          cancelled-100     loaded agent 100 in front of a standing shelf (cancelled), agent 99 behind it
          loaded-100-127    loaded agent 100 in front of the shelf that loaded agent id 127 carries away (not cancelled)
          delivers-127      (no structure: a delivery) loaded agent id 127 steps onto a goal with a requested shelf
  medium-70ag-global-scripted   one more trace, NOT random: the delivery-seeking policy of oracle/ref_runner.py, because random play on
      a crowded floor delivers next to nothing and the GLOBAL reward — paid to every agent, both slots — would never be seen

Everything runs under the pinned tie-break of oracle/ref_runner.py (lowest agent id among equal-depth predecessors).
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
import wide_fixtures as wf  # noqa: E402

P_ACT = [.05, .7, .1, .1, .05]
_TINY = dict(shelf_columns=3, column_height=8, shelf_rows=1)     # 11 x 10
_SMALL = dict(shelf_columns=3, column_height=8, shelf_rows=2)    # 20 x 10
_MEDIUM = dict(shelf_columns=5, column_height=8, shelf_rows=2)   # 20 x 16
_COMMON = dict(msg_bits=0, sensor_range=1, max_inactivity_steps=None, reward_type=1)
# name -> (constructor arguments, E envs, T steps, seed)
TRACES = {
    "tiny-65ag": (dict(_COMMON, **_TINY, n_agents=65, request_queue_size=20, max_steps=50), 2, 160, 31000),
    "small-127ag-twostage": (dict(_COMMON, **_SMALL, n_agents=127, request_queue_size=40, max_steps=45, reward_type=2), 2, 140, 32000),
    "medium-96ag-msg1-global-inact": (dict(_COMMON, **_MEDIUM, n_agents=96, request_queue_size=48, max_steps=60, max_inactivity_steps=25,
                                           msg_bits=1, reward_type=0), 2, 150, 33000),
    "imgdict-medium-100ag-sr2": (dict(_COMMON, **_MEDIUM, n_agents=100, request_queue_size=50, max_steps=40, sensor_range=2,
                                      observation_type=3), 2, 120, 34000),
    # (beside the four random traces: the delivery-seeking scripted policy of oracle/ref_runner.py, because random play on a crowded
    #  floor delivers next to nothing and the GLOBAL reward — every agent of the env, both slots — would never be paid)
    "medium-70ag-global-scripted": (dict(_COMMON, **_MEDIUM, n_agents=70, request_queue_size=35, max_steps=55, reward_type=0), 2, 120, 35000,
                                    "scripted"),
}
STRADDLE_KW = dict(_COMMON, **_SMALL, n_agents=127, request_queue_size=40, max_steps=500, reward_type=2)
STRADDLE_SEED = 2026


def reference_env(kw):
    wh = rr.load_reference()
    kw = dict(kw)
    kw["reward_type"] = wh.RewardType(int(kw["reward_type"]))
    kw["observation_type"] = wh.ObservationType(int(kw.get("observation_type", 1)))
    return wh.Warehouse(**kw)


def arrays_of(o):
    """(observation, features or None) of every agent of one env, as arrays"""
    if isinstance(o[0], dict):
        return np.stack([a["image"] for a in o]).astype(np.float32), np.stack([a["features"] for a in o]).astype(np.float32)
    return rr.obs_array(o), None


def small(a):
    return a.astype(np.int8 if a.max(initial=0) < 128 and a.min(initial=0) >= -128 else np.int16)


def record_trace(name, out_dir=HERE):
    kw, E, T, seed, *policy = TRACES[name]
    scripted = policy == ["scripted"]
    envs = [reference_env(kw) for _ in range(E)]
    N, M = kw["n_agents"], kw["msg_bits"]
    dict_obs = int(kw.get("observation_type", 1)) == 3
    state_keys = ("grid", "agent_x", "agent_y", "agent_dir", "agent_carry", "agent_delivered", "queue", "steps", "inactive", "rng") + \
        (("agent_msg",) if M else ())
    pol = np.random.default_rng(seed + 77)
    rec = {k: [] for k in state_keys + ("obs", "features", "rewards", "done", "actions", "was_reset")}
    first = [arrays_of(env.reset(seed=seed + e)[0]) for e, env in enumerate(envs)]
    init = {k: np.stack([rr.snapshot(env)[k] for env in envs]) for k in state_keys}
    prev_done = [False] * E
    deliveries = 0.0
    for t in range(T):
        row = {k: [] for k in rec}
        for e, env in enumerate(envs):
            a = [int(v) for v in (rr.scripted_actions(env, pol) if scripted else pol.choice(5, size=N, p=P_ACT))]
            if M:  # [Action, message bits...] per agent
                a = [[v] + [int(b) for b in pol.integers(0, 2, size=M)] for v in a]
            if prev_done[e]:  # NEXT_STEP autoreset: the step after `done` resets (no reseed), its action is ignored
                o, _ = env.reset()
                r, d = [0.0] * N, False
            else:
                o, r, d, _, _ = rr.ref_step(env, a)
            deliveries += sum(r)
            ob, ft = arrays_of(o)
            snap = rr.snapshot(env)
            for k in state_keys:
                row[k].append(snap[k])
            row["obs"].append(ob)
            if dict_obs:
                row["features"].append(ft)
            row["rewards"].append(np.asarray(r, np.float32))
            row["done"].append(np.uint8(d))
            row["actions"].append(np.asarray(a, np.int8))
            row["was_reset"].append(np.uint8(prev_done[e]))
            prev_done[e] = bool(d)
        for k, v in row.items():
            if v:
                rec[k].append(np.stack(v))
    out = {k: np.stack(v) for k, v in rec.items() if v}
    obs = out.pop("obs")
    assert int(out["grid"].max()) < 256
    out["grid"] = out["grid"].astype(np.uint8)
    for k in ("agent_x", "agent_y", "agent_dir", "agent_delivered", "agent_carry", "queue") + (("agent_msg",) if M else ()):
        out[k] = small(out[k])
    if dict_obs:
        out["features"] = out["features"].astype(np.uint8)
        out["features0"] = np.stack([f[1] for f in first]).astype(np.uint8)
    packed = dict(wf.pack_obs(obs, not dict_obs, 3))
    packed.update({"init_" + k: v for k, v in wf.pack_obs(np.stack([f[0] for f in first]), not dict_obs, 2).items()})
    fields = dict(out, **{f"init_{k}": v for k, v in init.items()})
    W = int(envs[0].grid_size[1])
    straddles = wf.trace_straddles(fields, W)
    resets = int(out["was_reset"].sum(0).min())
    assert straddles or scripted, f"{name}: no committed chain crosses agent index {wf.SLOT} — lengthen the trace or change its seed"
    assert resets >= 2, f"{name}: an env resets only {resets} times"
    assert not scripted or deliveries >= 2 * N, f"{name}: the scripted policy delivered {deliveries / N} shelves"
    meta = {
        "name": name, "env_id": None, "kwargs": dict(kw), "E": E, "T": T, "seed": seed, "obs_shape": list(obs.shape[3:]),
        "autoreset": "next_step", "tie_break": "lowest_agent_id", "gymnasium": "standin" if rr.using_standin_gymnasium() else "real",
        "reference": "semitable/robotic-warehouse (rware 2.0.0)", "deliveries": float(deliveries),
        "straddling_chains": len(straddles), "longest_straddling_chain": max([len(c) for _, _, c in straddles], default=0), "resets_per_env": resets,
    }
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **packed, **fields)
    print(f"{name}: N={N} E={E} T={T} deliveries={deliveries} resets>={resets} straddling chains {len(straddles)} "
          f"(longest {meta['longest_straddling_chain']}) -> {os.path.getsize(path) / 1024:.0f} KiB")
    return path


# ------------------------------------------------------------------------------------------------ the constructed states
LAST = 126   # index of agent id 127


def straddle_protos():
    """[(proto, agent indices of its slots)] on the 20 x 10 warehouse: highway rows y = 0, 9, 18, 19, highway columns x = 0, 3, 6, 9"""
    P = []
    P.append((cs._Proto("chain", "chain-62-65", "chain_3").chain((3, 0), [(4, 0), (5, 0), (6, 0), (7, 0)]), [62, 63, 64, 65]))
    ring = [(4, 9), (5, 9), (5, 10), (4, 10)]
    p = cs._Proto("cycle", "cycle-62-65", "cycle_4")
    for i, c in enumerate(ring):
        p.add(c, cs._dir_to(c, ring[(i + 1) % 4]))
    P.append((p, [62, 63, 64, 65]))
    P.append((cs._Proto("swap", "swap-0-64", "swap").add((4, 18), cs.RIGHT).add((5, 18), cs.LEFT), [0, 64]))
    P.append((cs._Proto("junction", "tie-3-70", "junction_tie").chain((6, 5), [(5, 5)]).chain((6, 5), [(6, 4)]), [3, 70]))
    P.append((cs._Proto("junction", "deeper-70-3", "junction_unequal").chain((6, 5), [(5, 5)]).chain((6, 5), [(6, 4), (6, 3)]), [3, 70, 71]))
    P.append((cs._Proto("blocked_head", "blocked-64", "chain_blocked_stationary").add((3, 12), cs.UP, cs.NOOP)
              .chain((3, 12), [(3, 13), (3, 14)]), [64, 63, 65]))
    P.append((cs._Proto("loaded", "cancelled-100", "chain_blocked_shelf").add((3, 3), cs.LEFT, cs.FORWARD, True)
              .chain((3, 3), [(4, 3)]), [100, 99]))
    P.append((cs._Proto("loaded", "loaded-100-127", "loaded_follows_loaded+chain_1").add((1, 3), cs.LEFT, cs.FORWARD, True)
              .add((2, 3), cs.LEFT, cs.FORWARD, True), [LAST, 100]))
    # (not a structure across the boundary: the one delivery the random traces cannot be asked for — made by the last agent)
    P.append((cs._Proto("loaded", "delivers-127", "chain_0").add((4, 18), cs.DOWN, cs.FORWARD, True), [LAST]))
    return P


def carry_requested(sc, base):
    """the loaded agent of `sc` carries the first REQUESTED shelf instead of the spare one _emit gave it (which goes home again)"""
    i = int(np.flatnonzero(sc["agent_carry"])[0])
    spare, want = int(sc["agent_carry"][i]) - 1, int(base["queue"][0]) - 1
    sc["shelf_xy"][want] = sc["shelf_xy"][spare]
    sc["shelf_xy"][spare] = base["shelf_xy"][spare]
    sc["agent_carry"][i] = want + 1


def record_straddle(out_dir=HERE):
    env = reference_env(STRADDLE_KW)
    env.reset(seed=STRADDLE_SEED)
    H, W = (int(v) for v in env.grid_size)
    N, S = env.n_agents, len(env.shelfs)
    base = dict(H=H, W=W, N=N, shelf_xy=np.array([[s.x, s.y] for s in env.shelfs], np.int32),
                queue=np.array([s.id for s in env.request_queue], np.int32))
    rng_state = env.np_random.bit_generator.state
    rng0 = rr.rng_state_tuple(env)
    scen = [cs._emit(p, ids, "boundary", base, H, W, N) for p, ids in straddle_protos()]
    carry_requested(next(sc for sc in scen if sc["variant"] == "delivers-127"), base)
    n, T = len(scen), cs.T_STEPS
    keys = ("agent_x", "agent_y", "agent_dir", "agent_carry", "agent_delivered")
    rec = {f"r_{k}": np.zeros((n, T, N), np.int16) for k in keys}
    rec.update(r_shelf_xy=np.zeros((n, T, S, 2), np.int16), r_queue=np.zeros((n, T, len(base["queue"])), np.int16),
               r_rewards_x2=np.zeros((n, T, N), np.int16), r_done=np.zeros((n, T), np.int16), r_req_action=np.zeros((n, T, N), np.int16))
    r_rng = np.zeros((n, T, 6), np.uint64)
    obs, classes = [], {}
    for k, sc in enumerate(scen):
        pins.inject_reference(env, sc, rng_state)
        cen = cs.census(sc, sc["actions"][0], H, W, cs.shelf_layer_from_xy(sc["shelf_xy"], H, W))
        assert cs.class_matches(cen, sc["claim"]), (sc["variant"], sc["claim"], dict(cen))
        for c, v in cen.items():
            classes[c] = classes.get(c, 0) + v
        o = [arrays_of(tuple(env._make_obs(a) for a in env.agents))[0]]
        for t in range(T):
            ot, rew, done, _, _ = rr.ref_step(env, [int(a) for a in sc["actions"][t]])
            o.append(arrays_of(ot)[0])
            snap = rr.snapshot(env)
            for key in keys:
                rec[f"r_{key}"][k, t] = snap[key]
            rec["r_shelf_xy"][k, t] = [[s.x, s.y] for s in env.shelfs]
            rec["r_queue"][k, t] = snap["queue"]
            rec["r_rewards_x2"][k, t] = np.round(np.asarray(rew, np.float64) * 2)
            rec["r_done"][k, t] = int(done)
            rec["r_req_action"][k, t] = [ag.req_action.value for ag in env.agents]
            r_rng[k, t] = snap["rng"]
        obs.append(np.stack(o))
        if sc["variant"] == "delivers-127":  # TWO_STAGE: half a reward at the goal, to the agent whose layer byte is 0xFF
            assert rec["r_rewards_x2"][k, 0, LAST] == 1 and rec["r_rewards_x2"][k, 0].sum() == 1
    out = {k: small(v) for k, v in rec.items()}
    for key in keys + ("shelf_xy", "queue", "actions"):
        out[key] = small(np.stack([sc[key] for sc in scen]))
    obs = np.stack(obs)
    out.update(wf.pack_obs(obs, True, 3))
    fam = [sc["family"] for sc in scen]
    meta = {
        "name": wf.STRADDLE, "env_id": None, "kwargs": dict(STRADDLE_KW), "H": H, "W": W, "N": int(N), "seed": STRADDLE_SEED, "n": n,
        "steps": T, "obs_shape": list(obs.shape[3:]), "tie_break": "lowest_agent_id",
        "gymnasium": "standin" if rr.using_standin_gymnasium() else "real", "reference": "semitable/robotic-warehouse (rware 2.0.0)",
        "agents": {sc["variant"]: ids for sc, (_, ids) in zip(scen, straddle_protos())}, "census_step0": dict(sorted(classes.items())),
    }
    path = os.path.join(out_dir, f"{wf.STRADDLE}.npz")
    np.savez_compressed(path, meta=json.dumps(meta), rng0=rng0, r_rng=r_rng,
                        family=np.array([cs.FAMILIES.index(f) for f in fam], np.int8),
                        ids=np.array([cs.ID_ASSIGNMENTS.index(sc["ids"]) for sc in scen], np.int8),
                        variant=np.array([sc["variant"] for sc in scen]), claim=np.array([sc["claim"] for sc in scen]), **out)
    print(f"{wf.STRADDLE}: N={N} scenarios={n} {meta['census_step0']} -> {os.path.getsize(path) / 1024:.0f} KiB")
    return path


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for trace in TRACES:
        if not only or trace in only:
            record_trace(trace)
    if not only or wf.STRADDLE in only:
        record_straddle()
