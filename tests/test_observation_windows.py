"""Observation windows and goal-cell counts pinned on CONSTRUCTED states (tests/observation_scenarios.py).

The expected answers in tests/golden/observations/*.npz were recorded from the unmodified reference (generate_observations.py):
the observation of the injected state and of two steps behind it, for every agent, with agents, shelves, queue, rewards, done
and the PCG64 words after each step.  Here the C oracle, the product sources under host-thread emulation and (GPU-marked) every
kernel path of the real engine replay them, exact.  A red test names task, scenario, family, step, agent and the window cell
(row, column, field) of the first differing element.
"""
import functools
import os
from collections import Counter

import numpy as np
import pytest

import observation_scenarios as osc
import pins
import ref_runner as rr
import rware_amd
from device_backends import emu_library
from rware_amd import _capi
from rware_amd.vector_env import global_image_from_state
from rware_oracle import OracleVecEnv

FIX_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observations")
LAYOUT_TASKS = [f"{p}layout-{g}" for g in ("1goal", "3goals", "5goals", "16goals") for p in ("", "img-")]
FLATTENED_TASKS = ["tiny-4ag", "tiny-9ag", "tiny-19ag", "tiny-3ag-sr2", "tiny-3ag-sr3", "tiny-3ag-sr4", "tiny-2ag-sr5", "tiny-3ag-msg1",
                   "tiny-3ag-msg2", "tiny-3ag-msg3-sr2", "small-3ag-normcoord", "29x28-10ag"] + [t for t in LAYOUT_TASKS if not t.startswith("img-")]
IMAGE_TASKS = ["img-tiny-3ag-directional-sr2", "img-tiny-3ag-northup", "img-square-4ag-all7", "imgdict-tiny-2ag"] + \
    [t for t in LAYOUT_TASKS if t.startswith("img-")]
TASKS = FLATTENED_TASKS + IMAGE_TASKS
REGISTERED = {"tiny-4ag": 16, "tiny-9ag": 8, "tiny-19ag": 8}   # ahead-of-time builds of the registered ids: envs per workgroup
RUNTIME_TASKS = ["tiny-3ag-sr2", "tiny-3ag-sr3", "tiny-3ag-sr4", "tiny-2ag-sr5", "tiny-3ag-msg1", "tiny-3ag-msg2", "tiny-3ag-msg3-sr2",
                 "29x28-10ag", "img-tiny-3ag-directional-sr2"] + LAYOUT_TASKS
AGENT_FIELDS = pins.AGENT_FIELDS
T = osc.T_STEPS


def unpack_observations(z):
    """z["obs"] (n, 3, N, ...) float32, z["features"] (IMAGE_DICT, else None); the flags the generator clears and does not store."""
    shape = tuple(z["meta"]["obs_shape"])
    if "obs_bits" in z:
        bits = np.unpackbits(z["obs_bits"], axis=-1)[..., :shape[-1] - 2]
        z["obs"] = np.concatenate([z["obs_xy"], bits.astype(np.float32)], axis=-1)
    else:
        n_el = int(np.prod(shape[1:]))
        flat = np.unpackbits(z["img_bits"], axis=-1)[..., :n_el] if "img_bits" in z else z["img_u8"]
        z["obs"] = flat.astype(np.float32).reshape(flat.shape[:2] + shape)
    z["features"] = z["feat_u8"].astype(np.float32) if "feat_u8" in z else None
    z["agent_delivered"] = np.zeros_like(z["agent_x"])


load = functools.partial(pins.load_npz, FIX_DIR, prepare=unpack_observations)


def kwargs_of(task, reward_type=None):
    meta = load(task)["meta"]
    kw = rware_amd.env_kwargs(meta["env_id"]) if meta["env_id"] else {}
    kw.update(meta["kwargs"])
    kw["reward_type"] = rware_amd.enums.enum_value(kw["reward_type"]) if reward_type is None else int(reward_type)
    return kw


def shape_of(task):
    meta = load(task)["meta"]
    orc = OracleVecEnv(1, **kwargs_of(task))
    sh = osc.make_shape(orc.hw, orc.goals, meta["N"], meta["Q"], meta["R"], meta["M"], goals_family=task in LAYOUT_TASKS)
    assert (sh["H"], sh["W"], sh["S"]) == (meta["H"], meta["W"], meta["S"])
    return sh


def state_of(z, k):
    return {f: z[f][k] for f in ("agent_x", "agent_y", "agent_dir", "agent_carry", "shelf_xy", "queue")}


def census_of(z, k, shape):
    return osc.window_census(state_of(z, k), shape, osc.msg_values(z["actions"][k, 0]))


def name_of(task, z, k, t):
    return (f"{task}, scenario {k} ({osc.FAMILIES[z['family'][k]]} / {z['variant'][k]}, ids {osc.ID_ASSIGNMENTS[z['ids'][k]]}, "
            f"reward type {int(z['reward_type'][k])}), {'the injected state' if t < 0 else f'step {t}'}")


FLAT_SELF = ("x", "y", "carrying", "dir UP", "dir DOWN", "dir LEFT", "dir RIGHT", "on highway")


def element_name(meta, index):
    """What an element of one agent's observation is: FLATTENED (e,) -> window cell (row, column, field); image (l, r, c)."""
    if len(index) == 1:
        e, CW, WIN = int(index[0]), 7 + meta["M"], 2 * meta["R"] + 1
        if e < 8:
            return f"self field '{FLAT_SELF[e]}'"
        cell, f = divmod(e - 8, CW)
        fields = ("has_agent", "dir UP", "dir DOWN", "dir LEFT", "dir RIGHT") + tuple(f"message bit {b}" for b in range(meta["M"])) + ("has_shelf", "requested")
        return f"window cell (row {cell // WIN}, column {cell % WIN}, field '{fields[f]}')"
    layer = (meta["kwargs"].get("image_observation_layers") or [0, 1, 2, 5, 6])[int(index[0])]
    names = ("SHELVES", "REQUESTS", "AGENTS", "AGENT_DIRECTION", "AGENT_LOAD", "GOALS", "ACCESSIBLE")
    return f"window cell (row {int(index[1])}, column {int(index[2])}, field 'layer {int(index[0])}: {names[layer]}')"


def split_obs(o):
    """(observation, features or None) from an oracle tuple, an env dict or a plain array."""
    if isinstance(o, dict):
        return np.asarray(o["image"]), np.asarray(o["features"])
    if isinstance(o, tuple):
        return np.asarray(o[0]), np.asarray(o[1])
    return np.asarray(o), None


def check_obs(task, z, idx, t, got, who, features=True):
    """Observation t (-1: of the injected state) of the batch idx against the fixture."""
    obs, feat = split_obs(got)
    want = z["obs"][idx, t + 1]
    assert obs.shape == want.shape, (who, obs.shape, want.shape)
    if not np.array_equal(obs, want):
        bad = np.argwhere(obs != want)[0]
        e, i = int(bad[0]), int(bad[1])
        raise AssertionError(f"{who}{name_of(task, z, int(idx[e]), t)} [batch row {e}]: agent {i}, {element_name(z['meta'], bad[2:])}: "
                             f"{obs[tuple(bad)]}, reference {want[tuple(bad)]}")
    if z["features"] is not None and features:
        wantf = z["features"][idx, t + 1]
        if not np.array_equal(feat, wantf):
            e, i, f = [int(v) for v in np.argwhere(feat != wantf)[0]]
            raise AssertionError(f"{who}{name_of(task, z, int(idx[e]), t)}: agent {i}, feature {f}: {feat[e, i, f]}, reference {wantf[e, i, f]}")


def check_state(task, z, idx, t, state, shelf_xy, rew, done, who):
    """Every recorded field: the agents (with their message where the task has message bits), shelves, queue, PCG64 words, rewards, done."""
    fields = AGENT_FIELDS + (("agent_msg",) if z["meta"]["M"] else ()) + ("shelf_xy", "queue", "rng")
    pins.check_state(task, z, idx, t, state, shelf_xy, rew, done, who, fields=fields, name_of=name_of)


check_rewards = functools.partial(pins.check_rewards, name_of=name_of)


def reward_groups(z, idx):
    """The scenarios idx by reward type (a constructor argument): [(reward type, sub-batch)], in first-seen order."""
    idx = np.asarray(idx)
    rts = z["reward_type"][idx]
    return [(int(rt), idx[rts == rt]) for rt in dict.fromkeys(int(v) for v in rts)]


def actions_of(z, idx, t=None):
    a = z["actions"][idx].astype(np.int32) if t is None else z["actions"][idx, t].astype(np.int32)
    return a if z["meta"]["M"] else a[..., 0]


def oracle_run(task, z, idx):
    for rt, sub in reward_groups(z, idx):
        orc = OracleVecEnv(len(sub), **kwargs_of(task, rt))
        check_obs(task, z, sub, -1, pins.inject(orc, z, sub), "oracle: ")
        for t in range(T):
            rew, done = orc.step(actions_of(z, sub, t))
            check_state(task, z, sub, t, orc.get_state(), orc.shelf_xy(), rew, done, "oracle: ")
            check_obs(task, z, sub, t, orc.obs(), "oracle: ")


def batch_of(sub, E=1, multiple=1, ragged=False):
    """The scenarios `sub` repeated E times, copy r rolled by r places — every scenario at every env slot of an E-env workgroup, every
    window row at every bit alignment its lane admits — padded with copies of the first one to a whole number of `multiple` envs
    (`ragged`: one env more, a partial last workgroup)."""
    return pins.pad_batch(np.concatenate([np.roll(sub, r) for r in range(E)]), multiple, ragged, fill=sub[0])


def engine_run(task, z, idx, fused, who, library=None, E=1, multiple=1, ragged=False, check_info=None, **ctor):
    """The engine on the injected batch against the fixture: the observation of the injected state (written by the refresh
    launch), per step every recorded field and the observation — a fused rollout hands back no state between its steps: there
    observations (IMAGE_DICT: the image tape — rollout() returns no features, so only the per-step runs compare them), rewards and done of
    every step, and the state behind the last one — then (per-step runs) restore() of a snapshot
    taken on the injected state, which writes that observation once more.  With `stats` the delivery counter against the
    recorded count."""
    for rt, sub in reward_groups(z, idx):
        env = None
        for _ in range(3):   # (E == "auto": the engine picks its geometry by shape AND batch size, so ask it until the batch is built for the answer)
            e_now = 16 if E == "auto" and env is None else int(env.engines[0].info.envs_per_workgroup) if E == "auto" else E
            if env is not None:
                env.close()
            rows = batch_of(sub, e_now, multiple, ragged)
            env = rware_amd.WarehouseVecEnv(len(rows), autoreset_mode="disabled", library=library, **kwargs_of(task, rt), **ctor)
            if E != "auto" or int(env.engines[0].info.envs_per_workgroup) == e_now:
                break
        try:
            assert int(env.engines[0].info.envs_per_workgroup) == e_now or E == 1, (task, env.engines[0].info.envs_per_workgroup, e_now)
            if check_info is not None:
                check_info(env.engines[0].info)
            unpack = env.unpack_obs if ctor.get("obs_format") == "packed" else (lambda o: o)
            check_obs(task, z, rows, -1, unpack(pins.inject(env, z, rows)), who)
            if fused:
                out = env.rollout(actions_of(z, rows).transpose((1, 0, 2, 3) if z["meta"]["M"] else (1, 0, 2)))
                obs, rew, term = out[0], out[1], out[2]
                for t in range(T):
                    check_obs(task, z, rows, t, unpack(obs[t]), who + "fused rollout: ", features=False)
                    check_rewards(task, z, rows, t, rew[t], term[t], who + "fused rollout: ")
                check_state(task, z, rows, T - 1, env.get_state(), env.shelf_xy(), rew[T - 1], term[T - 1], who + "fused rollout: ")
            else:
                token = env.snapshot()
                for t in range(T):
                    res = env.step(actions_of(z, rows, t))
                    check_state(task, z, rows, t, env.get_state(), env.shelf_xy(), res[1], res[2] | res[3], who)
                    check_obs(task, z, rows, t, unpack(res[0]), who)
                    if ctor.get("stats"):
                        got, want = env.event_counters()["deliveries"], z["r_deliveries"][rows, :t + 1].sum(-1)
                        assert np.array_equal(got, want), f"{who}{name_of(task, z, int(rows[np.argwhere(got != want)[0, 0]]), t)}: deliveries counted"
                check_obs(task, z, rows, -1, unpack(env.restore(token)), who + "restore(): ")
                env.free_snapshot(token)
        finally:
            env.close()


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_fixture_directory_stays_small():
    pins.check_fixture_directory_is_small(FIX_DIR, TASKS)


@pytest.mark.parametrize("task", TASKS)
def test_fixture_holds_every_class_its_shape_admits(task):
    """Per task: every scenario is a reachable state; the census of the injected states equals `meta`; it holds every class the
    shape admits — named here — and every family."""
    z = load(task)
    meta, shape = z["meta"], shape_of(task)
    N, S, R, M = meta["N"], meta["S"], meta["R"], meta["M"]
    WIN = 2 * R + 1
    total = Counter()
    for k in range(meta["n"]):
        osc.check_reachable(state_of(z, k), shape)
        assert np.all(z["actions"][k, 0, :, 0] == osc.NOOP) or osc.FAMILIES[z["family"][k]] == "goals", name_of(task, z, k, 0)
        total.update(census_of(z, k, shape))
    assert {osc.census_key(c): v for c, v in total.items()} == meta["census"]
    layout = task in LAYOUT_TASKS
    fam = Counter(osc.FAMILIES[f] for f in z["family"])
    assert dict(fam) == meta["families"]
    assert set(fam) == {"code_sweep", "self", "borders", "request_ids", "full_window"} | ({"messages"} if M else set()) | ({"goals"} if layout else set())
    # every window cell that lies on the grid for some observer, with each of the 15 codes
    need = {("cell", c, code) for c in range(WIN * WIN) if c != WIN * WIN // 2 and abs(c % WIN - R) < meta["W"] and abs(c // WIN - R) < meta["H"]
            for code in osc.CODES}
    assert len(osc.CODES) == 15 and len(need) == 15 * (WIN * WIN - 1)
    # every clip of the window the grid produces: 0 .. R columns / rows off each edge, both sides at once where the window is wider
    need |= {("clip",) + osc.clip_of(x, y, shape) for y in range(meta["H"]) for x in range(meta["W"])}
    if WIN > meta["W"]:
        # (an 11-wide window on the 10-wide grid: no observer column sees it whole — one column is off the grid at x = 4 and x = 5)
        assert all(c[1] + c[2] >= WIN - meta["W"] for c in need if c[0] == "clip")
    need |= {("self", d, l, h, r) for d in range(4) for l in (0, 1) for h in (0, 1) for r in ((0, 1) if l else (0,))}
    # requested and unrequested shelves at bits 0 and 31 of every request word and everywhere in the last word
    edge_ids = [s for s in range(1, S + 1) if (s & 31) in (0, 31) or (s >> 5) == (S >> 5)]
    assert {s for s in (31, 32, 63, 64, S - 1, S, 255, 256) if s <= S} <= set(edge_ids)
    need |= {(kind, s >> 5, s & 31) for s in edge_ids for kind in ("req", "unreq")}
    need |= {("lane", 1), ("lane", N), ("full_window", min(N - 1, WIN * WIN - 1))}
    if M:
        need |= {("msg", v) for v in range(1 << M)} | {("msg_at", cls, v) for cls in ("corner", "edge", "centre_row") for v in range(1 << M)}
    if layout:
        G = len(shape["goals"])
        need |= {("goal", g) for g in range(G)} | {("goals_held", k) for k in range(1, min(N, meta["Q"], G) + 1)}
    assert need <= set(total), (task, sorted(need - set(total), key=str)[:10])
    # the named request ids stand and are carried, requested and not, inside a window
    variants = set("+".join(str(v) for v in z["variant"][z["family"] == osc.FAMILIES.index("request_ids")]).split("+"))
    for s in osc.REQUEST_IDS + (S - 1, S):
        if 1 <= s <= S:
            assert {f"id{s}{a}{b}" for a in "sc" for b in "ru"} <= variants, (task, s)
    # every (cell, code) pair of the sweep under both id assignments — by the builder's own labels, and in the states themselves: a
    # neighbour seen by an observer with a lower and with a higher id (the observer's lane decides the bit alignment of its window
    # rows); with two agents, a cell without a neighbour seen by observer 0 and by observer 1 as well
    sweep = np.nonzero(z["family"] == osc.FAMILIES.index("code_sweep"))[0]
    cells = [(cl[1], cl[2]) for cl in need if cl[0] == "cell"]
    pairs = {f"c{c}k{code}" for c, code in cells}
    by = Counter()
    for a in (0, 1):
        ks = [k for k in sweep if z["ids"][k] == a]
        assert set("+".join(str(z["variant"][k]) for k in ks).split("+")) == pairs, (task, osc.ID_ASSIGNMENTS[a])
        for k in ks:
            by.update(osc.observer_order_census(state_of(z, k), shape))
    need_by = {("cell_by", order, c, code) for c, code in cells if code & 1 or N == 2 for order in (0, 1)}
    assert need_by <= set(by), (task, sorted(need_by - set(by))[:10])
    # simultaneous deliveries on goals of list index >= 2 only, under every reward type
    if layout:
        goals = z["family"] == osc.FAMILIES.index("goals")
        assert set(z["reward_type"][goals]) == {0, 1, 2} and meta["deliveries"] >= 3 * len(shape["goals"])
        if len(shape["goals"]) > 2:
            assert any(str(v).startswith("run2k") for v in z["variant"][goals])
        kmax = min(N, meta["Q"], len(shape["goals"]))
        assert int(z["r_deliveries"][goals].max()) == kmax, (task, kmax)


@pytest.mark.parametrize("task", TASKS)
def test_oracle_matches_reference_fixture(task):
    z = load(task)
    oracle_run(task, z, np.arange(z["meta"]["n"]))


@pytest.mark.skipif(not rr.reference_available(), reason="/root/reference not present")
@pytest.mark.parametrize("task", ["tiny-3ag-msg2", "img-tiny-3ag-directional-sr2", "layout-3goals"])
def test_reference_regenerates_the_committed_fixture(task, tmp_path):
    gen = pins.load_generator(os.path.join(FIX_DIR, "generate_observations.py"))
    pins.assert_regenerates(gen.record_task(task, str(tmp_path)), os.path.join(FIX_DIR, f"{task}.npz"))


def emulated_subset(task, z, limit):
    """A greedy cover: scenarios that together hold every census class of the fixture, every family and both id assignments."""
    shape = shape_of(task)
    per = []
    for k in range(z["meta"]["n"]):
        per.append(set(census_of(z, k, shape)) | {("fam", int(z["family"][k]), int(z["ids"][k]), int(z["reward_type"][k]))})
    left = set().union(*per)
    picked = []
    while left:
        k = max(range(len(per)), key=lambda j: len(per[j] & left))
        picked.append(k)
        left -= per[k]
    assert set().union(*(per[k] for k in picked)) == set().union(*per)
    assert len(picked) <= limit, (task, len(picked))
    return np.array(sorted(picked))


# The subset is a greedy cover of the census classes, at most 112 scenarios — except on the wide windows.  A class with a neighbour in it needs
# that neighbour on that cell, an env of N agents holds at most N (N - 1) of them, and a fixture has 12 x (WIN^2 - 1): at sensor ranges 4 and
# 5 that alone asks for 160 and 720 scenarios.  At ranges 2 and 3 the arithmetic would allow 48 and 96; the builder puts one observer-neighbour
# pair into a 3-agent env, not all six ordered pairs, so its cover comes to about 150 and 310.  More scenarios check no less: the limits below
# only keep the subsets from growing unnoticed.
EMU_LIMIT = {"tiny-3ag-sr2": 160, "img-tiny-3ag-directional-sr2": 160, "tiny-3ag-msg3-sr2": 160, "tiny-3ag-sr3": 330, "tiny-3ag-sr4": 540, "tiny-2ag-sr5": 960}
EMU_CASES = [(t, "generic", False) for t in TASKS] + [(t, "static", f) for t in ("tiny-4ag", "tiny-9ag") for f in (False, True)] + \
    [("tiny-19ag", "static", False)]


@pytest.mark.parametrize("task,build,fused", EMU_CASES, ids=[f"{t}-{b}-{'fused' if f else 'per_step'}" for t, b, f in EMU_CASES])
def test_emulated_engine_matches_reference_fixture(task, build, fused):
    """The product sources on host threads, on a subset that still holds every census class, family, id assignment and reward type
    (asserted in `emulated_subset`): the generic kernel, and the ahead-of-time build of the registered ids — register exchange
    (4 agents) and per-cell LDS exchange (9, 19), per step and, one task of each exchange kind, as a fused rollout."""
    z = load(task)
    idx = emulated_subset(task, z, EMU_LIMIT.get(task, 112))
    geom = dict(envs_per_workgroup=4, threads_per_workgroup=64, multiple=4) if build == "generic" else dict(multiple=16)

    def info(i):
        assert (i.build_kind == 0) == (build == "generic"), i.build_kind
    engine_run(task, z, idx, fused, f"emulated {build} kernel: ", library=emu_library(), check_info=info, **geom)


def test_more_than_16_goals_are_refused():
    kw = dict(shelf_columns=0, column_height=0, shelf_rows=0, n_agents=3, request_queue_size=3, max_steps=50, library=emu_library())
    rows = [".xxxxxxxx.", "gggggggggg"]
    with pytest.raises(_capi.EngineError) as ei:
        rware_amd.WarehouseVecEnv(4, layout="\n".join([rows[0], rows[1][:9] + ".", "gggggggg.."]), **kw)
    assert ei.value.code == _capi.RW_ERR_UNSUPPORTED and "more than 16 goal cells" in str(ei.value)
    env = rware_amd.WarehouseVecEnv(4, layout="\n".join([rows[0], rows[1][:9] + ".", "ggggggg..."]), **kw)
    assert len(env.goals) == 16
    env.close()


@pytest.mark.parametrize("task", TASKS)
def test_fixture_holds_what_random_play_reaches_and_more(task):
    """Random play on the oracle (p = [.05, .7, .1, .1, .05]; envs x steps by the table the figure was first measured with: 7 x 400 on the
    2-agent task of sensor range 1, 64 x 100 on the small warehouse, 16 x 200 on sensor ranges 2 .. 5 and everywhere else —
    generate_observations.floor_play): the census classes its states reach, beside the fixture's — the gap the fixture closes, not a
    tolerance.  Measured (classes random play reaches / classes the fixture holds):
    tiny-4ag 149 / 160, tiny-9ag 159 / 160, tiny-19ag 159 / 160, tiny-3ag-sr2 347 / 416, -sr3 646 / 800, -sr4 1040 / 1312,
    tiny-2ag-sr5 1297 / 1941, tiny-3ag-msg1 133 / 168, -msg2 154 / 176, -msg3-sr2 397 / 456, small-3ag-normcoord 168 / 196,
    29x28-10ag 174 / 208, img-tiny-3ag-directional-sr2 347 / 416, img-tiny-3ag-northup 141 / 160, img-square-4ag-all7 215 / 216,
    imgdict-tiny-2ag 116 / 160, layouts (FLATTENED and IMAGE alike): 1 goal 168 / 170, 3 goals 172 / 178, 5 goals 172 / 180,
    16 goals 178 / 199.  With 9 and 19 agents only the full window is out of random play's reach.  The classes do not cross a
    cell's code with the observer's lane or the env's slot in its workgroup: the census test asserts every (cell, code) pair under
    both id orders, and the GPU tests run every scenario at every env slot."""
    z = load(task)
    meta, shape = z["meta"], shape_of(task)
    played = osc.random_play_classes(OracleVecEnv(meta["floor"]["envs"], **kwargs_of(task)), shape, meta["floor"]["steps"])
    held = {tuple(int(v) if v.lstrip("-").isdigit() else v for v in key.split("/")) for key in meta["census"]}
    print(f"floor {task}: random play reaches {len(set(played) & held)} of the fixture's {len(held)} classes")
    assert set(played) <= held, (task, sorted(set(played) - held, key=str)[:10])
    assert len(set(played)) < len(held)
    assert meta["floor"]["classes_random_play"] == len(set(played) & held) and meta["floor"]["classes_fixture"] == len(held)


# ------------------------------------------------------------------------------------------------------------------ GPU
def all_of(z):
    return np.random.default_rng(11).permutation(z["meta"]["n"])


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["per_step", "fused"])
@pytest.mark.parametrize("task", TASKS)
def test_gpu_default_build_matches_reference_fixture(task, fused):
    """The build the engine picks — the ahead-of-time one for the registered ids (build kind and geometry asserted) — with every
    scenario at every env slot of a workgroup."""
    z = load(task)
    E = REGISTERED.get(task, "auto")

    def info(i):
        if task in REGISTERED:
            assert i.build_kind in (1, 2) and i.jit == 0 and i.envs_per_workgroup == E, (i.build_kind, i.jit, i.envs_per_workgroup)
    engine_run(task, z, all_of(z), fused, "default build: ", E=E, multiple=32, check_info=info)


@pytest.mark.gpu
@pytest.mark.parametrize("task", TASKS)
def test_gpu_generic_kernel_matches_reference_fixture(task):
    z = load(task)

    def info(i):
        assert i.build_kind == 0 and i.jit == 0 and i.envs_per_workgroup == 4, (i.build_kind, i.jit, i.envs_per_workgroup)
    engine_run(task, z, all_of(z), False, "generic kernel: ", E=4, multiple=4, ragged=True, check_info=info,
               envs_per_workgroup=4, threads_per_workgroup=64, jit="off")   # (from 4096 envs on the engine would ask for a run-time build first)


@pytest.mark.gpu
@pytest.mark.parametrize("task", RUNTIME_TASKS)
def test_gpu_runtime_build_matches_reference_fixture(task, tmp_path, monkeypatch):
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    z = load(task)
    def info(i):
        assert i.build_kind == 1 and i.jit in (1, 2), (i.build_kind, i.jit)
    for fused in (False, True):
        engine_run(task, z, all_of(z), fused, "run-time exact-shape build: ", E="auto", multiple=32, check_info=info, jit="force")


@pytest.mark.gpu
@pytest.mark.parametrize("task", FLATTENED_TASKS)
def test_gpu_packed_observations_match_reference_fixture(task):
    z = load(task)
    def info(i):
        assert i.obs_packed == 1
    engine_run(task, z, all_of(z), False, "packed rows: ", E="auto", multiple=32, check_info=info, obs_format="packed")


@pytest.mark.gpu
@pytest.mark.parametrize("task", IMAGE_TASKS)
def test_gpu_uint8_images_match_reference_fixture(task):
    z = load(task)
    def info(i):
        assert i.obs_packed == 2
    engine_run(task, z, all_of(z), False, "uint8 images: ", E="auto", multiple=32, check_info=info, obs_format="uint8")


@pytest.mark.gpu
@pytest.mark.parametrize("task", ["tiny-4ag", "layout-3goals"])
def test_gpu_opt_in_build_matches_reference_fixture(task):
    """Action masks, episode statistics, event counters and time-limit truncation at once: the RW_STATS_BUILD text of the same gather.
    The delivery counter must equal the recorded count (the goals family delivers 1 .. 3 shelves in one step)."""
    z = load(task)
    flags = dict(action_mask=True, episode_stats=True, stats=True, time_limit_truncates=True)
    def info(i):
        assert i.stats & 15 == 15, i.stats
    engine_run(task, z, all_of(z), False, "opt-in build: ", E="auto", multiple=32, check_info=info, **flags)


def _layout_env(task, backend, B, **ctor):
    if backend == "emulated":
        ctor.update(library=emu_library(), envs_per_workgroup=4, threads_per_workgroup=64)
    return rware_amd.WarehouseVecEnv(B, autoreset_mode="disabled", **kwargs_of(task), **ctor)


@pytest.mark.parametrize("backend", ["emulated", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("task", [t for t in LAYOUT_TASKS if t.startswith("img-")])
def test_global_image_goals_layer_on_the_injected_states(task, backend):
    """rw_global_image's goal lookup for 1, 3, 5 and 16 goals: the GOALS layer (ImageLayer value 5, the fourth of the default layers),
    float32 and uint8, on every injected state."""
    GOALS = rware_amd.enums.ImageLayer.GOALS
    z = load(task)
    idx = np.arange(z["meta"]["n"]) if backend == "gpu" else emulated_subset(task, z, 112)
    rows = batch_of(idx, multiple=4)
    env = _layout_env(task, backend, len(rows))
    try:
        pins.inject(env, z, rows)
        want = global_image_from_state(env.get_state(), env.goals, [GOALS])
        assert want.sum() == len(rows) * len(env.goals)
        for dtype in ("float32", "uint8"):
            got = env.global_image_device([GOALS], dtype=dtype)
            assert got.dtype == np.dtype(dtype) and np.array_equal(got, want), (task, dtype, np.argwhere(got != want)[:3].tolist())
    finally:
        env.close()


@pytest.mark.parametrize("backend", ["emulated", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("task", [t for t in LAYOUT_TASKS if t.startswith("img-")])
def test_reset_observation_shows_every_goal(task, backend):
    """The reset launch's own GOALS layer (IMAGE): after reset(seed=...) and, two steps later, after a masked reset, against the oracle."""
    B = 32 if backend == "emulated" else 256
    env = _layout_env(task, backend, B)
    try:
        orc = OracleVecEnv(B, **kwargs_of(task))
        got, want = env.reset(seed=31)[0], orc.reset(seed=31)
        assert np.array_equal(got, want), (task, np.argwhere(got != want)[:3].tolist())
        layers = kwargs_of(task)["image_observation_layers"]
        assert want[:, :, layers.index(5)].sum() > 0
        rng = np.random.default_rng(2)
        for _ in range(2):
            a = rng.integers(0, 5, size=(B, orc.N)).astype(np.int32)
            env.step(a)
            orc.step(a)
        mask = (np.arange(B) % 3 != 1)
        got = env.reset(mask=mask)[0]
        orc.reset(mask=mask.astype(np.uint8))
        want = orc.obs()
        assert np.array_equal(got, want), (task, np.argwhere(got != want)[:3].tolist())
    finally:
        env.close()
