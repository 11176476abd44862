"""Collision resolution pinned on CONSTRUCTED chains, cycles, swaps and junctions (tests/collision_scenarios.py).

The expected answers in tests/golden/collisions/*.npz were recorded from the unmodified reference (generate_collisions.py, pinned
tie-break); here the C oracle, the product sources under host-thread emulation and (GPU-marked) every kernel path of the real engine
replay them: 4 steps per scenario, every recorded field, exact.  A red test names task, scenario, family, id assignment, step and agent.
"""
import functools
import os
from collections import Counter

import numpy as np
import pytest

import collision_scenarios as cs
import pins
import ref_runner as rr
import rware_amd
from engine_checks import default_envs_per_workgroup
from rware_oracle import OracleVecEnv

FIX_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collisions")
TASKS = [f"tiny-{n}ag" for n in (2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 19)] + ["small-4ag", "small-16ag"]
AGENT_FIELDS = pins.AGENT_FIELDS
FIELDS = AGENT_FIELDS + ("shelf_xy", "queue")     # what check_state compares beside rewards and done: all the generator records
T = cs.T_STEPS
name_of = cs.name_of
load = functools.partial(pins.load_npz, FIX_DIR)
check_state = functools.partial(pins.check_state, fields=FIELDS, name_of=name_of)


def kwargs_of(task):
    kw = rware_amd.env_kwargs(load(task)["meta"]["env_id"])
    kw["reward_type"] = rware_amd.enums.enum_value(kw["reward_type"])
    return kw


def step0_census(z, k):
    H, W = z["meta"]["H"], z["meta"]["W"]
    st = {f: z[f][k] for f in AGENT_FIELDS}
    return cs.analyse(st["agent_x"], st["agent_y"], st["agent_dir"], st["agent_carry"], z["actions"][k, 0], H, W,
                      cs.shelf_layer_from_xy(z["shelf_xy"][k], H, W))


def oracle_run(task, z, idx):
    """The oracle on the injected batch: [observation of the injected state, (obs, rewards, done) per step], checked against the
    fixture on the way."""
    orc = OracleVecEnv(len(idx), **kwargs_of(task))
    out = [pins.inject(orc, z, idx)]
    for t in range(z["meta"]["steps"]):
        rew, done = orc.step(z["actions"][idx, t].astype(np.int32))
        check_state(task, z, idx, t, orc.get_state(), orc.shelf_xy(), rew, done, who="oracle: ")
        out.append((orc.obs(), rew, done))
    return out


def engine_run(task, z, idx, fused, who, library=None, **ctor):
    """pins.engine_run against the fixture (every recorded field, every step) and the oracle (observations, rewards, done); with
    `stats` the failed-move counter behind step 0 against the requests the reference turned down."""
    def failed_moves(env, t):
        if t == 0 and ctor.get("stats"):
            want = ((z["actions"][idx, 0] == cs.FORWARD) & (z["r_req_action"][idx, 0] == cs.NOOP)).sum(-1)
            pins.check_same(task, z, idx, 0, "failed_moves", env.event_counters()["failed_moves"], want, who, name_of=name_of)
    return pins.engine_run(task, z, idx, fused, who, kwargs_of(task), oracle_run(task, z, idx), fields=FIELDS, name_of=name_of,
                           library=library, after_step=failed_moves, **ctor)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_fixture_directory_stays_small():
    pins.check_fixture_directory_is_small(FIX_DIR, TASKS)


@pytest.mark.parametrize("task", TASKS)
def test_fixture_holds_every_class_and_every_family_yields_its_claim(task):
    """Per task: the census of every scenario's step 0 holds the class its family claims (a generator bug that builds a
    non-collision cannot pass); every family, id assignment and every census class that fits N agents is present; `meta` lists
    the counts."""
    z = load(task)
    meta, N = z["meta"], z["meta"]["N"]
    total = Counter()
    for k in range(meta["n"]):
        cen, _ = step0_census(z, k)
        total.update(cen)
        assert cs.class_matches(cen, str(z["claim"][k])), f"{name_of(task, z, k, 0)}: the census found {dict(cen)}"
    assert dict(sorted(total.items())) == meta["census_step0"]
    fam = Counter(cs.FAMILIES[f] for f in z["family"])
    assert dict(fam) == {f: c for f, c in meta["families"].items() if c}
    need_fam = {"chain", "blocked_head", "swap", "junction", "loaded"} | ({"head_loses"} if N >= 3 else set()) | ({"cycle"} if N >= 4 else set())
    assert need_fam <= set(fam), (task, fam)
    for f in need_fam - {"loaded"}:
        got = {cs.ID_ASSIGNMENTS[i] for i in z["ids"][z["family"] == cs.FAMILIES.index(f)]}
        assert got == set(cs.ID_ASSIGNMENTS), (task, f, got)
    need = {"swap", "chain_blocked_stationary", "chain_blocked_shelf", "junction_tie", "loaded_follows_loaded"} | {f"chain_{d}" for d in range(N)}
    if N >= 3:
        need |= {"swap_tail", "junction_unequal"}
    if N >= 4:      # (a loser with a follower needs two agents, and two more to tie with it)
        need |= {f"cycle_{k}" for k in range(4, N + 1, 2)} | {"head_loses"}
    if N >= 5:      # (three in the main branch, one in the other, one from the side)
        need |= {f"cycle_{k}_tail" for k in range(4, N, 2)} | {"junction_nested"}
    assert need <= set(total), (task, sorted(need - set(total)))
    # structures the thinning sample must never drop: junction cells in corners and on borders (the per-cell kernels' neighbour
    # masks), the deep N - 2 against 0 junction, nested junctions in the winning and in the losing branch
    variants = [str(v) for v in z["variant"]]
    prefixes = (["corner_", "border_", "deep_"] if N >= 3 else []) + (["nested_winner"] if N >= 5 else []) + (["nested_loser"] if N >= 8 else [])
    for pre in prefixes:
        assert any(v.startswith(pre) for v in variants), (task, pre)
    # consecutive chain members on both sides of every encoding boundary, and the last index in front of index 0
    for a, b in ((5, 6), (11, 12), (12, 13), (15, 16), (N - 1, 0)):
        if max(a, b) < N:
            hit = 0
            for k in np.nonzero(z["ids"] == cs.ID_ASSIGNMENTS.index("boundary"))[0]:
                xa, ya, xb, yb = z["agent_x"][k, a], z["agent_y"][k, a], z["agent_x"][k, b], z["agent_y"][k, b]
                d = z["agent_dir"][k, b]
                hit += int((xb + cs.DXY[int(d)][0], yb + cs.DXY[int(d)][1]) == (xa, ya) and z["actions"][k, 0, b] == cs.FORWARD)
            assert hit >= 1, (task, a, b)


@pytest.mark.parametrize("task", TASKS)
def test_oracle_matches_reference_fixture(task):
    z = load(task)
    oracle_run(task, z, np.arange(z["meta"]["n"]))


@pytest.mark.skipif(not rr.reference_available(), reason="/root/reference not present")
@pytest.mark.parametrize("task", ["tiny-5ag", "tiny-9ag"])
def test_reference_regenerates_the_committed_fixture(task, tmp_path):
    gen = pins.load_generator(os.path.join(FIX_DIR, "generate_collisions.py"))
    pins.assert_regenerates(gen.record_task(task, str(tmp_path)), os.path.join(FIX_DIR, f"{task}.npz"))


@pytest.mark.skipif(not rr.reference_available(), reason="/root/reference not present")
@pytest.mark.parametrize("task", ["tiny-7ag", "tiny-17ag"])
def test_census_predicts_who_moves_in_the_live_reference(task):
    """Every scenario, every step: the agents the census says move (its classes under the pinned rule) are the agents that
    change cell in the live reference — stepped here, not read from the fixture."""
    z = load(task)
    meta = z["meta"]
    H, W = meta["H"], meta["W"]
    env = rr.make_reference_env(meta["env_id"])
    env.reset(seed=meta["seed"])
    for k in range(meta["n"]):
        pins.inject_reference(env, {f: z[f][k] for f in AGENT_FIELDS + ("shelf_xy", "queue")})
        for t in range(T):
            snap = rr.snapshot(env)
            _, movers = cs.analyse(snap["agent_x"], snap["agent_y"], snap["agent_dir"], snap["agent_carry"], z["actions"][k, t], H, W,
                                   snap["grid"][1])
            rr.ref_step(env, [int(a) for a in z["actions"][k, t]])
            moved = {i for i, ag in enumerate(env.agents) if (ag.x, ag.y) != (snap["agent_x"][i], snap["agent_y"][i])}
            assert moved == movers, f"{name_of(task, z, k, t)}: the reference moved {sorted(moved)}, the census predicts {sorted(movers)}"


def emulated_subset(z, limit):
    """At most `limit` scenarios that hold every census class of the fixture (two of each where there are), every family and
    every id assignment."""
    per, picked = {}, []
    for k in range(z["meta"]["n"]):
        keys = list(step0_census(z, k)[0]) + [("fam", int(z["family"][k]), int(z["ids"][k]))]
        if any(per.get(c, 0) < 2 for c in keys):
            picked.append(k)
            for c in keys:
                per[c] = per.get(c, 0) + 1
    assert len(picked) <= limit, len(picked)
    rest = [k for k in range(z["meta"]["n"]) if k not in set(picked)]
    more = np.random.default_rng(5).permutation(len(rest))[:limit - len(picked)]
    return np.array(sorted(picked + [rest[i] for i in more]))


@pytest.mark.parametrize("build,fused", [("generic", False), ("static", False), ("static", True)],
                         ids=["generic-per_step", "static-per_step", "static-fused"])
@pytest.mark.parametrize("task", ["tiny-4ag", "tiny-6ag", "tiny-9ag", "tiny-13ag"])
def test_emulated_engine_matches_reference_fixture(task, build, fused):
    """The product sources on host threads: the generic kernel (one text for per-step launches and rollouts: per-step only) and the
    ahead-of-time build of the task — register exchange; per-cell exchange for the per-step launches of 9 and 13 agents, which is
    why those run both launch forms — on a subset that holds every census class, family and id assignment.  The subset is small
    because a workgroup is 256 OS threads here; the whole fixture runs on the oracle and on the GPU."""
    from engine_backend import build_emu
    z = load(task)
    idx = emulated_subset(z, 112)
    assert len(idx) % 16 == 0
    geom = dict(envs_per_workgroup=4, threads_per_workgroup=64) if build == "generic" else {}
    info = engine_run(task, z, idx, fused, f"emulated {build} kernel: ", library=build_emu(), **geom)
    assert (info.build_kind == 0) == (build == "generic")


# ------------------------------------------------------------------------------------------------------------------ GPU
def gpu_batch(z, multiple, ragged=False):
    """All scenarios, shuffled with a fixed seed (different structures share a wavefront), padded with copies of scenario 0 to a
    whole number of `multiple` envs — or, `ragged`, to one env more than that: a partial last workgroup."""
    return pins.pad_batch(np.random.default_rng(11).permutation(z["meta"]["n"]), multiple, ragged)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["per_step", "fused"])
@pytest.mark.parametrize("task", TASKS)
def test_gpu_ahead_of_time_build_matches_reference_fixture(task, fused):
    """(rw_info names the build and its geometry, not the agent-phase variant: that the per-step launches of 9 .. 19 agents take the
    per-cell exchange follows from the kernel text — kCell = per-step launch of a static build with N >= 9 — not from an assert.)"""
    z = load(task)
    N = z["meta"]["N"]
    info = engine_run(task, z, gpu_batch(z, 32), fused, "ahead-of-time build: ")
    assert info.build_kind in (1, 2) and info.jit == 0 and info.envs_per_workgroup == default_envs_per_workgroup(task, N), \
        (info.build_kind, info.jit, info.envs_per_workgroup)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["per_step", "fused"])
def test_gpu_8_env_geometry_of_16_agents_matches_reference_fixture(fused):
    """13 .. 16 agents have two per-step geometries on the small warehouse: the 4-env one is the default here (above), this is the other."""
    z = load("small-16ag")
    info = engine_run("small-16ag", z, gpu_batch(z, 32), fused, "8-env build: ", envs_per_workgroup=8, threads_per_workgroup=256)
    assert info.build_kind == 2 and info.jit == 0 and info.envs_per_workgroup == 8


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["per_step", "fused"])
@pytest.mark.parametrize("task", TASKS)
def test_gpu_generic_kernel_matches_reference_fixture(task, fused):
    z = load(task)
    idx = gpu_batch(z, 4, ragged=True)          # (the generic kernel takes any batch: the last workgroup holds one env)
    assert len(idx) % 4 == 1
    info = engine_run(task, z, idx, fused, "generic kernel: ", envs_per_workgroup=4, threads_per_workgroup=64)
    assert info.build_kind == 0 and info.jit == 0 and info.envs_per_workgroup == 4


@pytest.mark.gpu
@pytest.mark.parametrize("task", ["tiny-6ag", "tiny-12ag", "tiny-19ag"])
def test_gpu_runtime_build_matches_reference_fixture(task, tmp_path, monkeypatch):
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    z = load(task)
    for fused in (False, True):
        info = engine_run(task, z, gpu_batch(z, 32), fused, "run-time exact-shape build: ", jit="force")
        assert info.build_kind == 1 and info.jit in (1, 2), (info.build_kind, info.jit)


@pytest.mark.gpu
@pytest.mark.parametrize("task", ["tiny-4ag", "tiny-16ag"])
def test_gpu_packed_observations_match_reference_fixture(task):
    z = load(task)
    info = engine_run(task, z, gpu_batch(z, 4), False, "generic kernel, packed rows: ", envs_per_workgroup=4, threads_per_workgroup=64,
                      obs_format="packed")
    assert info.build_kind == 0 and info.obs_packed == 1


@pytest.mark.gpu
def test_gpu_failed_move_counter_matches_reference_fixture():
    z = load("tiny-9ag")
    info = engine_run("tiny-9ag", z, gpu_batch(z, 8), False, "event counters: ", stats=True)
    # (the ahead-of-time builds of the gfx950 library carry no counting code: below 4096 envs the generic kernel steps)
    assert info.stats == 1 and info.build_kind == 0 and info.jit == 0, (info.stats, info.build_kind, info.jit)


# ---------------------------------------------------------------------------------------------- a measured floor for random play
FLOOR_TASKS = ["rware-tiny-9ag-v1", "rware-tiny-13ag-v1", "rware-tiny-19ag-v1", "rware-small-16ag-v1"]


@pytest.mark.parametrize("backend", ["oracle", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("env_id", FLOOR_TASKS)
def test_dense_repacking_reaches_the_rare_structures(env_id, backend):
    """150 steps of FORWARD-heavy play; every 10 steps all agents are re-packed into a dense block by state injection
    (collision_scenarios.pack_dense).  The census of the oracle's pre-step states must reach the floors below — conditions on the
    INPUTS, which the oracle alone decides — and (GPU) the engine must match the oracle on every env and step."""
    kw = rware_amd.env_kwargs(env_id)
    kw["reward_type"] = rware_amd.enums.enum_value(kw["reward_type"])
    B, N = 96, kw["n_agents"]
    orc = OracleVecEnv(B, **kw)
    o2 = orc.reset(seed=17)
    env = None
    if backend == "gpu":
        env = rware_amd.WarehouseVecEnv(B, autoreset_mode="disabled", **kw)
        assert env.engines[0].info.build_kind == 2
        assert np.array_equal(env.reset(seed=17)[0], o2)
    H, W = orc.H, orc.W
    rng = np.random.default_rng(99)
    total = Counter()
    for t in range(150):
        if t % 10 == 0:
            st, sxy = orc.get_state(), orc.shelf_xy()
            for e in range(B):
                x, y, d = cs.pack_dense(rng, st["agent_x"][e], st["agent_y"][e], st["agent_dir"][e], st["agent_carry"][e], st["grid"][e, 1], H, W)
                st["agent_x"][e], st["agent_y"][e], st["agent_dir"][e] = x, y, d
                for i in np.nonzero(st["agent_carry"][e])[0]:
                    sxy[e, st["agent_carry"][e, i] - 1] = (x[i], y[i])
            fields = {f: st[f] for f in ("agent_x", "agent_y", "agent_dir")}
            orc.set_state(**fields)
            orc.recalc_grid(sxy)
            if env is not None:
                env.set_state(refresh_obs=False, **fields)
                env.recalc_grid(sxy)
        p = 0.9 if t % 10 == 0 else 0.8
        a = rng.choice(5, size=(B, N), p=[(1 - p) / 4, p] + [(1 - p) / 4] * 3).astype(np.int32)
        st = orc.get_state()
        for e in range(B):
            total.update(cs.analyse(st["agent_x"][e], st["agent_y"][e], st["agent_dir"][e], st["agent_carry"][e], a[e], H, W, st["grid"][e, 1])[0])
        rew, done = orc.step(a)
        if env is not None:
            obs, r1, term, _, _ = env.step(a)
            o2 = orc.obs()
            if not (np.array_equal(obs, o2) and np.array_equal(r1, rew) and np.array_equal(term, done.astype(bool))):
                e = int(np.argwhere((obs != o2).reshape(B, -1).any(-1) | (r1 != rew).any(-1) | (term != done.astype(bool)))[0, 0])
                cen = cs.analyse(st["agent_x"][e], st["agent_y"][e], st["agent_dir"][e], st["agent_carry"][e], a[e], H, W, st["grid"][e, 1])
                raise AssertionError(f"{env_id}, step {t}, env {e}: engine and oracle differ; this env's step holds {dict(cen[0])}, movers "
                                     f"{sorted(cen[1])}; x {st['agent_x'][e].tolist()} y {st['agent_y'][e].tolist()} dir {st['agent_dir'][e].tolist()} "
                                     f"carry {st['agent_carry'][e].tolist()} actions {a[e].tolist()}")
    if env is not None:
        se, so = env.get_state(), orc.get_state()
        for k in so:
            assert np.array_equal(se[k], so[k]), (env_id, k)
        env.close()
    got = dict(cycle=sum(v for k, v in total.items() if k.startswith("cycle_") and not k.endswith("_tail")),
               cycle_tail=sum(v for k, v in total.items() if k.startswith("cycle_") and k.endswith("_tail")),
               junction_unequal=total["junction_unequal"],
               deep_chain=sum(v for k, v in total.items() if k.startswith("chain_") and k[6:].isdigit() and 2 * int(k[6:]) >= N))
    print(f"census {env_id}: {got} | {dict(sorted(total.items()))}")
    assert got["cycle"] >= 50 and got["cycle_tail"] >= 20 and got["junction_unequal"] >= 50 and got["deep_chain"] >= 20, (env_id, got)
