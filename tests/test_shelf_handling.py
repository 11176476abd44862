"""What a step does after the moves are committed — TOGGLE_LOAD, the goal loop, request replacement, the three reward types, the two
counters and the termination test — pinned on CONSTRUCTED states (tests/handling_scenarios.py).

The expected answers in tests/golden/handling/*.npz were recorded from the unmodified reference (generate_handling.py) under four
configurations: the three reward types with small limits, and TWO_STAGE with no limit.  Here the C oracle, the product sources under
host-thread emulation and (GPU-marked) every kernel path of the real engine replay them: 6 steps per scenario, every recorded field —
the agents with `has_delivered`, every shelf, the queue, both counters, the generator words, rewards, done — exact.  A red test names
task, scenario, family, claim, id assignment, reward type, step and agent.
"""
import functools
import json
import os
from collections import Counter

import numpy as np
import pytest

import handling_scenarios as hs
import lockstep
import pins
import ref_runner as rr
import rng_states as rs
import rware_amd
import wide_fixtures as wf
from device_backends import emu_library
from engine_checks import default_envs_per_workgroup
from models import EpisodeModel, bits, mask_model, same_buffers
from rware_oracle import OracleVecEnv

FIX_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handling")
REGISTERED = [f"tiny-{n}ag" for n in (2, 4, 8, 9, 13, 16, 19)] + ["small-4ag", "small-16ag"]
WIDE = "tiny-65ag"                                   # more than 64 agents: no oracle, the fixture holds the observations
TASKS = REGISTERED + ["small-20ag", "29x28-10ag", "layout-5goals", WIDE]
ORACLE_TASKS = [t for t in TASKS if t != WIDE]
C = len(hs.CONFIGS)
T = hs.T_STEPS
AGENT_FIELDS = pins.AGENT_FIELDS
FIELDS = AGENT_FIELDS + ("shelf_xy", "queue", "steps", "inactive", "rng")     # what check_state compares beside rewards and done
OPT_IN = dict(stats=True, episode_stats=True, action_mask=True, time_limit_truncates=True)
_views = {}


load = functools.partial(pins.load_npz, FIX_DIR, prepare=wf.unpack_scenario_obs)


def generator():
    return pins.load_generator(os.path.join(FIX_DIR, "generate_handling.py"))


def config_name(c):
    rt, limited = hs.CONFIGS[c]
    return f"reward type {rt} ({('GLOBAL', 'INDIVIDUAL', 'TWO_STAGE')[rt]})" + ("" if limited else ", no limits")


def view(task, c):
    """The fixture under configuration c in the form tests/pins.py replays: r_<field>[scenario, step]; `config` says which it is."""
    key = (task, c)
    if key not in _views:
        z = load(task)
        assert all(z[k].shape[1:3] == (C, T) for k in hs.PER_CONFIG), task
        _views[key] = hs.config_view(z, c)
    return _views[key]


def name_of(task, v, k, t):
    return (f"{task}, scenario {k} ({hs.FAMILIES[v['family'][k]]} / {v['variant'][k]}, claims {v['claim'][k]}), "
            f"ids {hs.ID_ASSIGNMENTS[v['ids'][k]]}, {config_name(v['config'])}, step {t}")


check_state = functools.partial(pins.check_state, fields=FIELDS, name_of=name_of)
check_same = functools.partial(pins.check_same, name_of=name_of)


def kwargs_of(task, c, **more):
    """Constructor arguments of the task under configuration c: ONE dict for the env and the oracle."""
    meta = load(task)["meta"]
    kw = lockstep.oracle_kwargs(meta["env_id"], **meta["overrides"])
    kw.update(hs.config_shape({}, c))     # (the reward type and both limits)
    kw.update(more)
    return kw


def shape_of(task, c=None):
    z = load(task)
    m = z["meta"]
    sh = dict(H=m["H"], W=m["W"], N=m["N"], S=m["S"], Q=m["Q"], goals=[tuple(g) for g in m["goals"]], highways=z["highways"],
              shelf_xy=rs.shelf_home(z["highways"]), queue=z["queue0"], rng0=z["rng0"])
    return sh if c is None else hs.config_shape(sh, c)


def states_of(task, k, c):
    """[state before step 0, after step 0, ... after step T - 1] of scenario k under configuration c, as the census reads them."""
    z = load(task)
    first = dict({f: z[f][k] for f in AGENT_FIELDS + ("shelf_xy", "queue", "steps", "inactive")})
    out = [first]
    for t in range(T):
        st = {f: z["r_" + f][k, t] for f in AGENT_FIELDS[:4] + ("shelf_xy", "queue")}
        st.update({f: z["r_" + f][k, c, t] for f in ("agent_delivered", "steps", "inactive")})
        out.append(st)
    return out


_census = {}


def census_of(task, k, c):
    """The census of every step of scenario k under configuration c (computed once)."""
    if (task, k, c) not in _census:
        z, sh, sts = load(task), shape_of(task, c), states_of(task, k, c)
        _census[task, k, c] = [hs.handling_census(sts[t], z["actions"][k, t], sts[t + 1], z["r_choice"][k, t], sh) for t in range(T)]
    return _census[task, k, c]


# ------------------------------------------------------------------------------------------------------------------ runners
def check_events(task, v, idx, t, deliveries, failed_moves, base, who=""):
    """Running event counters against the recorded `choice` counts and failed moves of steps 0 .. t."""
    for what, got, rec in (("deliveries", deliveries, v["r_choice"]), ("failed_moves", failed_moves, v["r_failed"])):
        want = rec[idx, :t + 1].sum(1) + base[what]
        if not np.array_equal(np.asarray(got), want):
            e = int(np.argwhere(np.asarray(got) != want)[0, 0])
            raise AssertionError(f"{who}{name_of(task, v, int(idx[e]), t)}: {what} {int(np.asarray(got)[e]) - int(base[what][e])} since the injection, "
                                 f"reference {int(want[e]) - int(base[what][e])}")


def oracle_run(task, c, idx, corrupt=None):
    """The oracle on scenarios idx under configuration c, every field of every step against the fixture — the agents with their flags,
    the shelves, the queue, both counters, the generator words, rewards, done, and its event counters against the recorded counts.
    `corrupt` = (field, step): one element of that field is changed behind that step, and nothing else (the sensitivity test).
    Returns what pins.engine_run compares an engine with: [observation of the injected state, (obs, rewards, done) per step]."""
    v = view(task, c)
    orc = OracleVecEnv(len(idx), **kwargs_of(task, c))
    out = [pins.inject(orc, v, idx)]
    base = dict(deliveries=orc.stat_deliveries.copy(), failed_moves=orc.stat_failed_moves.copy())

    def bent(field, t, a):
        if corrupt != (field, t):
            return a
        a = np.array(a)
        a.flat[a.size // 2] = 1 - a.flat[a.size // 2] if field == "done" else a.flat[a.size // 2] + 1
        return a

    for t in range(T):
        rew, done = orc.step(v["actions"][idx, t].astype(np.int32))
        st = orc.get_state()
        st = {f: bent(f, t, a) for f, a in st.items()}
        check_state(task, v, idx, t, st, bent("shelf_xy", t, orc.shelf_xy()), bent("rewards", t, rew), bent("done", t, done), who="oracle: ")
        check_events(task, v, idx, t, bent("deliveries", t, orc.stat_deliveries), bent("failed_moves", t, orc.stat_failed_moves), base, "oracle: ")
        out.append((orc.obs(), rew, done))
    return out


def engine_run(task, c, idx, fused, who, library=None, **ctor):
    """The engine on scenarios idx under configuration c: pins.engine_run — every recorded field against the fixture, observations,
    rewards and done against the oracle, itself checked against the fixture on the way — or, where no oracle exists, against the
    fixture's own observations."""
    v = view(task, c)
    want = oracle_run(task, c, idx) if v["meta"]["N"] <= 64 else pins.fixture_outputs(v, idx)
    return pins.engine_run(task, v, idx, fused, f"{who}{config_name(c)}: ", kwargs_of(task, c), want, fields=FIELDS, name_of=name_of,
                           library=library, **ctor)


def opt_in_run(task, c, idx, who, library=None, **ctor):
    """One engine with the event counters, the episode statistics, the action mask and the time-limit split all on (configurations with
    limits only): every step against the fixture as ever, `terminated` / `truncated` against the rule that fired in the reference's
    counters, the event counters against the recorded counts, the episode buffers against EpisodeModel fed with the recorded rewards and
    ends, the mask against mask_model on the engine's own (checked) state."""
    v = view(task, c)
    assert hs.CONFIGS[c][1]
    who = f"{who}{config_name(c)}: "
    B, N = len(idx), v["meta"]["N"]
    env = rware_amd.WarehouseVecEnv(B, autoreset_mode="disabled", library=library, **kwargs_of(task, c), **OPT_IN, **ctor)
    try:
        pins.inject(env, v, idx)
        ev = env.event_counters()
        base = dict(deliveries=ev["deliveries"].copy(), failed_moves=ev["failed_moves"].copy())
        model = EpisodeModel(B, N, "disabled")
        first = env.episode_stats()
        for k in ("return", "length", "last_return", "last_length", "count"):     # (whatever reset() and the injection left)
            model.v[k][...] = first[k]
        hw = np.asarray(env.highways)
        check_same(task, v, idx, 0, "action mask of the injected state", env.action_mask(), bits(mask_model(env.get_state(), hw)[0]), who)
        for t in range(T):
            obs, rew, term, trunc, _ = env.step(v["actions"][idx, t].astype(np.int32))
            st = env.get_state()
            check_state(task, v, idx, t, st, env.shelf_xy(), rew, term | trunc, who)
            want_term = v["r_inactive"][idx, t] >= hs.LIMITS["max_inactivity_steps"]
            want_trunc = v["r_steps"][idx, t] >= hs.LIMITS["max_steps"]
            assert np.array_equal(want_term | want_trunc, v["r_done"][idx, t].astype(bool))
            check_same(task, v, idx, t, "terminated (the inactivity rule)", term, want_term, who)
            check_same(task, v, idx, t, "truncated (the step limit)", trunc, want_trunc, who)
            ev = env.event_counters()
            check_events(task, v, idx, t, ev["deliveries"], ev["failed_moves"], base, who)
            model.step(v["r_rewards_x2"][idx, t].astype(np.float32) / 2, v["r_done"][idx, t].astype(bool))
            same_buffers(env.episode_stats(), model, f"{who}{task}, step {t}")
            check_same(task, v, idx, t, "action mask", env.action_mask(), bits(mask_model(st, hw)[0]), who)
        return env.engines[0].info
    finally:
        env.close()


def autoreset_run(task, c, idx, mode, who, library=None, **ctor):
    """Scenarios idx under an autoreset mode, against OracleVecEnv.step_autoreset: the ends the injected counters bring about are followed
    by a reset step (next_step) or a fresh episode (same_step) — observations, rewards, done, terminal observations, and every field of
    the state behind every step."""
    v = view(task, c)
    kw = kwargs_of(task, c)
    env = rware_amd.WarehouseVecEnv(len(idx), autoreset_mode=mode, library=library, **kw, **ctor)
    orc = OracleVecEnv(len(idx), **kw)
    try:
        lockstep.same_obs(pins.inject(env, v, idx), pins.inject(orc, v, idx), f"{who}{task}: the observation of the injected state")
        run = lockstep.lockstep(env, orc, v["actions"][idx].astype(np.int32).transpose(1, 0, 2), mode, seed=None, state_every=1)
        assert run.episodes >= len(idx) // 4, (task, mode, run)
        return env.engines[0].info
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_fixture_directory_stays_small():
    pins.check_fixture_directory_is_small(FIX_DIR, TASKS)


@pytest.mark.parametrize("task", TASKS)
def test_fixture_holds_every_class_and_every_scenario_its_claim(task):
    """Per task: the builder rebuilds the injected states of the fixture; every scenario's census holds its claim under every
    configuration; every family and class the geometry admits, every id assignment N admits (in every family that has an acting
    agent), every reward type and every handled shelf id is present; `meta` lists the counts."""
    z = load(task)
    meta, N, S = z["meta"], z["meta"]["N"], z["meta"]["S"]
    scen = hs.build_scenarios(shape_of(task), seed=meta["round_seed"])
    assert len(scen) == meta["n"]
    for f in AGENT_FIELDS + ("shelf_xy", "queue", "steps", "inactive", "rng", "actions"):
        assert np.array_equal(np.stack([sc[f] for sc in scen]), z[f]), (task, f)
    assert [sc["claim"] for sc in scen] == z["claim"].tolist() and [sc["variant"] for sc in scen] == z["variant"].tolist()
    total = [Counter() for _ in range(C)]
    for k in range(meta["n"]):
        for c in range(C):
            by_step = census_of(task, k, c)
            assert hs.claim_holds(by_step, str(z["claim"][k]), hs.CONFIGS[c][1]), \
                f"{name_of(task, view(task, c), k, 0)}: the census found {[dict(b) for b in by_step]}"
            for b in by_step:
                total[c].update(b)
    assert [dict(sorted(t.items())) for t in total] == meta["census"]
    families, classes = hs.admitted(shape_of(task))
    fam = Counter(hs.FAMILIES[f] for f in z["family"])
    assert dict(fam) == {f: n for f, n in meta["families"].items() if n} and families <= set(fam), (task, fam)
    held = set().union(*total)
    assert classes <= held, (task, sorted(classes - held))
    assert {rt for rt, _ in hs.CONFIGS} == {0, 1, 2} and [list(cf) for cf in hs.CONFIGS] == meta["configs"]
    ids = [a for a in hs.ID_ASSIGNMENTS if a == "lowest" or (N >= 2 and (a == "highest" or int(a[1:].split("_")[1]) < N))]
    assert {a: n for a, n in meta["id_assignments"].items() if n} == dict(Counter(hs.ID_ASSIGNMENTS[i] for i in z["ids"]))
    for f in set(fam):
        got = {hs.ID_ASSIGNMENTS[i] for i in z["ids"][z["family"] == hs.FAMILIES.index(f)]}
        assert got == set(ids), (task, f, got)
    # the acting agents really sit on both sides of the boundary an assignment is named after
    acting = (z["actions"] != hs.NOOP).any(1)
    for a in ids[2:]:
        lo, hi = (int(b) for b in a[1:].split("_"))
        rows = acting[z["ids"] == hs.ID_ASSIGNMENTS.index(a)]
        assert rows[:, lo].any() and (rows[:, lo] & rows[:, hi]).any(), (task, a)
    assert N < 2 or acting[z["ids"] == hs.ID_ASSIGNMENTS.index("highest")][:, N - 1].any()
    handled = {s for s in hs.HANDLED_IDS + (S - 1, S) if 1 <= s <= S}
    carried = set(np.unique(z["agent_carry"])) | set(np.unique(z["r_agent_carry"]))
    assert handled <= carried, (task, sorted(handled - carried))
    # toggle against mover, `_then_leaves`: the load the toggle left decides the mover's next step (handling_scenarios, family 6)
    leaves = [k for k in range(meta["n"]) if "_then_leaves_" in str(z["variant"][k])]
    assert leaves or task not in REGISTERED or N < 2, task
    for k in leaves:
        mover, occupant = int(np.flatnonzero(z["actions"][k, 0] == hs.FORWARD)[0]), int(np.flatnonzero(z["actions"][k, 0] == hs.TOGGLE)[0])
        at = lambda t, i: (int(z["r_agent_x"][k, t, i]), int(z["r_agent_y"][k, t, i]))      # noqa: E731
        start, cell = (int(z["agent_x"][k, mover]), int(z["agent_y"][k, mover])), (int(z["agent_x"][k, occupant]), int(z["agent_y"][k, occupant]))
        assert at(0, mover) == start and at(0, occupant) == cell and at(1, occupant) != cell, (task, k)
        if "_picks_" in str(z["variant"][k]):
            assert z["r_agent_carry"][k, 0, occupant] and at(1, mover) == cell, (task, k, "the mover follows the loaded occupant into its cell")
        else:
            assert not z["r_agent_carry"][k, 0, occupant] and all(at(t, mover) == start for t in range(T)), \
                (task, k, "the mover stays out of the cell the unloaded occupant left")


@pytest.mark.parametrize("task", ORACLE_TASKS)
def test_oracle_matches_reference_fixture(task):
    for c in range(C):
        oracle_run(task, c, np.arange(load(task)["meta"]["n"]))


@pytest.mark.skipif(not rr.reference_available(), reason="/root/reference not present")
@pytest.mark.parametrize("task", ["tiny-9ag", "layout-5goals"])
def test_reference_regenerates_the_committed_fixture(task, tmp_path):
    pins.assert_regenerates(generator().record_task(task, str(tmp_path)), os.path.join(FIX_DIR, f"{task}.npz"))


def test_fixtures_hold_every_class_the_golden_traces_hold():
    """The census over every committed trace of the reference (random and scripted play), printed; the constructed fixtures hold every
    class, so at least every class that play reached — now, and when trace_census.json was recorded.  Only the inclusion is asserted:
    a trace added later makes the stored record stale (said in the output, with how to re-record it), not the test red."""
    gen = generator()
    with open(os.path.join(FIX_DIR, "trace_census.json")) as f:
        stored = json.load(f)
    per = {name: dict(sorted(gen.trace_census(meta, z).items())) for name, meta, z in gen.golden_traces()}
    total = Counter()
    for cen in per.values():
        total.update(cen)
    print(f"census of {len(per)} golden traces, {total['env_steps']} env-steps: {dict(sorted(total.items()))}")
    if per != stored["traces"] or dict(total) != stored["total"]:
        print("tests/golden/handling/trace_census.json no longer matches the committed traces: re-record it with "
              "`python tests/golden/handling/generate_handling.py trace_census`")
    held, admitted = set(), set()
    for task in TASKS:
        held |= set().union(*(Counter(cen) for cen in load(task)["meta"]["census"]))
        admitted |= hs.admitted(shape_of(task))[1]
    assert admitted <= held
    for what, reached in (("the committed traces", set(total)), ("trace_census.json", set(stored["total"]))):
        assert reached - {"env_steps"} <= held, (what, sorted(reached - {"env_steps"} - held))


def emulated_subset(task, limit=112, per_config=(32, 32, 32, 16)):
    """[(configuration, scenarios)]: at most `limit` (scenario, configuration) pairs that hold every census class of the fixture, every
    family under every id assignment and every configuration, twice where there are two — chosen as
    tests/test_collision_structures.emulated_subset does, per configuration filled up to a multiple of 16 and shuffled so that
    neighbouring envs differ."""
    z = load(task)
    n = z["meta"]["n"]
    keys_of, holders = {}, {}
    for k in range(n):
        for c in range(C):
            keys_of[k, c] = {cl for b in census_of(task, k, c) for cl in b} | {("fam", int(z["family"][k]), int(z["ids"][k])), ("config", c)}
            for key in keys_of[k, c]:
                holders.setdefault(key, []).append((k, c))
    per, picked = Counter(), {c: [] for c in range(C)}
    need = lambda kc: sum(per[key] < min(2, len(holders[key])) for key in keys_of[kc])      # noqa: E731  (keys this pair still helps)
    for j, key in enumerate(sorted(holders, key=lambda key: (len(holders[key]), str(key)))):      # the rarest first
        while per[key] < min(2, len(holders[key])):
            room = [(k, c) for k, c in holders[key] if k not in picked[c] and len(picked[c]) < per_config[c]]
            if not room:
                break
            k, c = min(room, key=lambda kc: (-need(kc), (kc[1] - j) % C, kc[0]))      # the pair that fills most; the configurations in turn
            picked[c].append(k)
            per.update(keys_of[k, c])
    rng = np.random.default_rng(5)
    out = []
    for c in range(C):
        rest = [k for k in rng.permutation(n).tolist() if k not in set(picked[c])]
        idx = np.array(picked[c] + rest[:(-len(picked[c])) % 16], np.int64)
        out.append((c, rng.permutation(idx)))
    assert sum(len(i) for _, i in out) <= limit and all(len(i) % 16 == 0 for _, i in out)
    return out


def test_emulated_subset_holds_every_class_family_assignment_and_reward_type():
    """On every task the emulated engine test runs: each census class, each (family, id assignment) and each configuration is held by two
    (scenario, configuration) pairs of the subset, or by the only one the whole fixture has."""
    for task in dict.fromkeys(t for t, _, _ in EMULATED):
        z = load(task)
        sub = emulated_subset(task)
        keys = lambda k, c: ({cl for b in census_of(task, k, c) for cl in b}                                        # noqa: E731
                             | {("fam", int(z["family"][k]), int(z["ids"][k])), ("config", c)})
        exist, held = Counter(), Counter()
        for k in range(z["meta"]["n"]):
            for c in range(C):
                exist.update(keys(k, c))
        for c, idx in sub:
            assert len(idx) >= 16 and len(set(idx.tolist())) == len(idx), (task, c)
            for k in idx:
                held.update(keys(int(k), c))
        assert set().union(*(Counter(cen) for cen in z["meta"]["census"])) <= set(exist) and set(range(C)) == {c for c, _ in sub}
        short = {str(key): (held[key], n) for key, n in exist.items() if held[key] < min(n, 2)}
        assert not short, (task, short)


def wavefront_groups(task):
    """Scenarios that must not share a wavefront with the others.  The exact-shape kernels decide per WAVEFRONT whether any of its envs
    may deliver — a prefilter from registers (`had`: a shelf on goal 0 / 1 at the start of the step; four flags: a loaded mover arrived
    at, or left, goal 0 / 1) — and every env of a wavefront in which one may takes the full goal loop.  In a shuffled batch a neighbour's
    arrival therefore rescues an env whose own prefilter is wrong.  Two groups, each run as a batch of its own:
      had_only   some step delivers, and at no step a loaded agent moves onto or off goal 0 / 1: the deliveries hang on `had` alone
      quiet      no shelf stands on goal 0 / 1 behind any step: every step takes the register copy of the counters and the termination test
    Both with the scenarios of the limits family first."""
    z = load(task)
    goals = np.array(z["meta"]["goals"][:2])
    x = np.concatenate([z["agent_x"][:, None], z["r_agent_x"]], 1).astype(np.int32)      # (n, 1 + T, N)
    y = np.concatenate([z["agent_y"][:, None], z["r_agent_y"]], 1).astype(np.int32)
    carry = np.concatenate([z["agent_carry"][:, None], z["r_agent_carry"]], 1)
    on_goal = ((x[..., None] == goals[:, 0]) & (y[..., None] == goals[:, 1])).any(-1)
    moved = (x[:, 1:] != x[:, :-1]) | (y[:, 1:] != y[:, :-1])
    flags = (moved & (carry[:, :-1] != 0) & (on_goal[:, 1:] | on_goal[:, :-1])).any((1, 2))
    shelf_on_goal = ((z["r_shelf_xy"][..., None, 0] == goals[:, 0]) & (z["r_shelf_xy"][..., None, 1] == goals[:, 1])).any((1, 2, 3))
    limits_first = lambda idx: np.array(sorted(idx.tolist(), key=lambda k: (z["family"][k] != hs.FAMILIES.index("limits"), k)), np.int64)  # noqa: E731
    return dict(had_only=limits_first(np.flatnonzero(~flags & (z["r_choice"] > 0).any(1))), quiet=limits_first(np.flatnonzero(~shelf_on_goal)))


def group_batch(idx, multiple, limit=None):
    """The group's scenarios (its first `limit`), filled up to a whole number of `multiple` envs with its own members."""
    idx = idx[:limit]
    return np.concatenate([idx, idx[:(-len(idx)) % multiple]])


def test_wavefront_groups_hold_what_they_are_for():
    for task in REGISTERED:
        z, g = load(task), wavefront_groups(task)
        held = {name: set().union(*(set(b) for k in idx for c in range(C) for b in census_of(task, int(k), c))) for name, idx in g.items()}
        assert {"delivery_in_place", "delivery_nobody_on_goal", "delivery_standing_under_unloaded_agent", "two_deliveries", "chained_delivery",
                "max_steps_due_with_delivery", "max_inactivity_steps_due_with_delivery"} <= held["had_only"], (task, sorted(held["had_only"]))
        assert {"max_steps_due_without_delivery", "max_inactivity_steps_due_without_delivery", "both_limits_due", "max_steps_one_before",
                "max_inactivity_steps_one_before", "max_steps_none_counter_near_2_30", "drop", "pick"} <= held["quiet"], (task, sorted(held["quiet"]))
        assert not any(cl.startswith("delivery") for cl in held["quiet"]) and not any("arrival" in cl for cl in held["had_only"])
        assert len(g["had_only"]) >= 32 and len(g["quiet"]) >= 32 and (z["family"][g["quiet"][:10]] == hs.FAMILIES.index("limits")).all()


EMULATED = [("tiny-4ag", "generic", False), ("tiny-4ag", "static", False), ("tiny-4ag", "static", True),
            ("tiny-8ag", "generic", False), ("tiny-8ag", "static", False), ("tiny-8ag", "static", True),
            ("tiny-9ag", "generic", False), ("tiny-9ag", "static", False), ("tiny-9ag", "static", True),
            ("tiny-13ag", "generic", False), ("tiny-13ag", "static", False), ("tiny-13ag", "static", True),
            (WIDE, "generic", False)]


@pytest.mark.parametrize("task,build,fused", EMULATED, ids=[f"{t}-{b}-{'fused' if f else 'per_step'}" for t, b, f in EMULATED])
def test_emulated_engine_matches_reference_fixture(task, build, fused):
    """The product sources on host threads: the generic kernel, and the ahead-of-time build of the task per step and fused (register
    agent phase up to 8 agents; per-cell exchange for the per-step launches of 9 and 13) — which take an engine with the limits
    overridden — on a subset that holds every class, family, id assignment and configuration.  The whole fixture runs on the oracle
    and on the GPU."""
    geom = dict(envs_per_workgroup=4, threads_per_workgroup=64) if build == "generic" else {}
    if task == WIDE:
        geom = dict(envs_per_workgroup=4, threads_per_workgroup=256, jit="off")
    for c, idx in emulated_subset(task):
        info = engine_run(task, c, idx, fused, f"emulated {build} kernel: ", library=emu_library(), **geom)
        assert (info.build_kind == 0) == (build == "generic"), (info.build_kind, c)


@pytest.mark.parametrize("fused", [False, True], ids=["per_step", "fused"])
@pytest.mark.parametrize("task", ["tiny-4ag", "tiny-8ag", "tiny-13ag"])
def test_emulated_prefilter_alone_in_its_wavefront(task, fused):
    """wavefront_groups on host threads: 32 scenarios of either group, under every configuration, on the ahead-of-time build."""
    for name, idx in wavefront_groups(task).items():
        for c in range(C):
            info = engine_run(task, c, group_batch(idx, 16, 32), fused, f"emulated static kernel, {name} alone: ", library=emu_library())
            assert info.build_kind != 0


def test_emulated_opt_in_outputs_match_the_reference_fixture():
    """(the GPU test below, on host threads, for one configuration: the generic kernel carries the opt-in code)"""
    z = load("tiny-4ag")
    idx = np.random.default_rng(3).permutation(z["meta"]["n"])[:32]
    opt_in_run("tiny-4ag", 2, idx, "emulated, opt-in outputs: ", library=emu_library())


@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_emulated_limit_family_under_autoreset(mode):
    idx = group_batch(limit_family("tiny-4ag"), 16)       # (all of the family, the copies under the other id assignments included)
    autoreset_run("tiny-4ag", 0, idx, mode, "emulated: ", library=emu_library())


SENSITIVE = AGENT_FIELDS + ("shelf_xy", "queue", "steps", "inactive", "rng", "rewards", "done", "deliveries", "failed_moves")


@pytest.mark.parametrize("field", SENSITIVE)
def test_one_corrupted_element_fails_the_check(field):
    """The check behind every runner of this module, on the oracle: unperturbed it passes (test_oracle_matches_reference_fixture); with
    ONE element of ONE compared field changed behind ONE step it raises and names scenario, family, claim, id assignment, reward type
    and that step."""
    idx = np.arange(load("tiny-4ag")["meta"]["n"])
    for step in (0, T - 1):
        with pytest.raises(AssertionError) as err:
            oracle_run("tiny-4ag", 2, idx, corrupt=(field, step))
        msg = str(err.value)
        assert msg.startswith("oracle: tiny-4ag, scenario ") and f"step {step}" in msg and "reward type 2 (TWO_STAGE)" in msg, msg
        assert all(word in msg for word in ("claims ", "ids ", " / ")), msg
        if field in AGENT_FIELDS + ("rewards",):
            assert "agent " in msg, msg


# ------------------------------------------------------------------------------------------------------------------ GPU
def limit_family(task):
    z = load(task)
    return np.flatnonzero(z["family"] == hs.FAMILIES.index("limits"))


def gpu_batch(task, multiple, ragged=False):
    """All scenarios, shuffled with a fixed seed (different situations share a wavefront), padded with copies of scenario 0 to a whole
    number of `multiple` envs — or, `ragged`, to one env more than that: a partial last workgroup."""
    return pins.pad_batch(np.random.default_rng(11).permutation(load(task)["meta"]["n"]), multiple, ragged)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["per_step", "fused"])
@pytest.mark.parametrize("task", REGISTERED)
def test_gpu_ahead_of_time_build_matches_reference_fixture(task, fused):
    N = load(task)["meta"]["N"]
    for c in range(C):
        info = engine_run(task, c, gpu_batch(task, 32), fused, "ahead-of-time build: ")
        assert info.build_kind in (1, 2) and info.jit == 0 and info.envs_per_workgroup == default_envs_per_workgroup(task, N), \
            (info.build_kind, info.jit, info.envs_per_workgroup)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["per_step", "fused"])
@pytest.mark.parametrize("task", REGISTERED)
def test_gpu_prefilter_alone_in_its_wavefront(task, fused):
    """wavefront_groups: every scenario of either group, in batches that hold nothing else."""
    for name, idx in wavefront_groups(task).items():
        for c in range(C):
            info = engine_run(task, c, group_batch(idx, 32), fused, f"ahead-of-time build, {name} alone: ")
            assert info.build_kind in (1, 2) and info.jit == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["per_step", "fused"])
def test_gpu_8_env_geometry_of_16_agents_matches_reference_fixture(fused):
    for c in range(C):
        info = engine_run("small-16ag", c, gpu_batch("small-16ag", 32), fused, "8-env build: ", envs_per_workgroup=8, threads_per_workgroup=256)
        assert info.build_kind == 2 and info.jit == 0 and info.envs_per_workgroup == 8


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["per_step", "fused"])
@pytest.mark.parametrize("task", TASKS)
def test_gpu_generic_kernel_matches_reference_fixture(task, fused):
    idx = gpu_batch(task, 4, ragged=True)          # (the generic kernel takes any batch: the last workgroup holds one env)
    assert len(idx) % 4 == 1
    geom = dict(envs_per_workgroup=4, threads_per_workgroup=256 if task == WIDE else 64)
    for c in range(C):
        info = engine_run(task, c, idx, fused, "generic kernel: ", jit="off", **geom)
        assert info.build_kind == 0 and info.jit == 0 and info.envs_per_workgroup == 4


@pytest.mark.gpu
@pytest.mark.parametrize("task", ["tiny-8ag", "tiny-13ag", "small-20ag", "layout-5goals"])
def test_gpu_runtime_build_matches_reference_fixture(task, tmp_path, monkeypatch):
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    for c in range(C):
        for fused in (False, True):
            info = engine_run(task, c, gpu_batch(task, 32), fused, "run-time exact-shape build: ", jit="force")
            assert info.build_kind == 1 and info.jit in (1, 2), (info.build_kind, info.jit)


@pytest.mark.gpu
@pytest.mark.parametrize("task", ["tiny-4ag", "small-16ag"])
def test_gpu_packed_observations_match_reference_fixture(task):
    for c in range(C):
        info = engine_run(task, c, gpu_batch(task, 4), False, "generic kernel, packed rows: ", envs_per_workgroup=4, threads_per_workgroup=64,
                          obs_format="packed")
        assert info.build_kind == 0 and info.obs_packed == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
@pytest.mark.parametrize("task,ctor", [(t, {}) for t in REGISTERED] + [("tiny-13ag", dict(envs_per_workgroup=4, threads_per_workgroup=64))],
                         ids=REGISTERED + ["tiny-13ag-generic"])
def test_gpu_limit_family_under_autoreset(task, ctor, mode):
    """Every scenario of the limits family — the copies under the other id assignments included — filled up with the family's own first
    members to whole workgroups (the generic constructor: 4 envs each)."""
    family = limit_family(task)
    idx = group_batch(family, 4 if ctor else 32)
    assert set(idx.tolist()) == set(family.tolist()) and len(idx) % (4 if ctor else 32) == 0
    for c in range(3):
        info = autoreset_run(task, c, idx, mode, "", **ctor)
        assert (info.build_kind == 0) == bool(ctor)


@pytest.mark.gpu
@pytest.mark.parametrize("task,ctor", [(t, {}) for t in ORACLE_TASKS] + [("tiny-9ag", dict(jit="force"))], ids=ORACLE_TASKS + ["tiny-9ag-jit"])
def test_gpu_opt_in_outputs_match_the_reference_fixture(task, ctor, tmp_path, monkeypatch):
    """One engine per reward type with `stats`, `episode_stats`, `action_mask` and `time_limit_truncates` all on."""
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    for c in range(3):
        info = opt_in_run(task, c, gpu_batch(task, 8), "opt-in outputs: ", **ctor)
        assert info.stats and (info.jit in (1, 2)) == bool(ctor), (info.stats, info.build_kind, info.jit)
