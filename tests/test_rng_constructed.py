"""The four numpy-exact draws of the engine — agent cells, directions and request queue at reset(), the replacement request after a
delivery — pinned on CONSTRUCTED PCG64 states (tests/rng_states.py): states built by inverting the LCG step so that the next draws
reject, sit on a threshold boundary, yield an extreme value or consume nothing.  Seeded play does not get there: for n = 47 a
rejection needs one of 42 values out of 2^32.

numpy is the reference of the draws themselves (the oracle's restatement and the Python tracer against Generator.integers /
Generator.choice, value and all six state words); the unmodified reference recorded tests/golden/rng_edges/*.npz
(generate_rng_edges.py), which the oracle, the product sources under host-thread emulation and (GPU-marked) every kernel path replay.
Everything is compared exactly; a red test names task, scenario, claim, field and index.
"""
import functools
import os

import numpy as np
import pytest

import pins
import ref_runner as rr
import rng_states as rs
import rware_amd
from device_backends import emu_library
from lockstep import lockstep, oracle_kwargs, same_obs, same_state
from rware_oracle import OracleVecEnv, lib

FIX_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rng_edges")
TASKS = list(rs.TASKS)
REGISTERED = [t for t in TASKS if not rs.TASKS[t][1]]


def delivery_step_as_step_0(z):
    """the one step of the delivery scenarios in the form pins.check_rewards reads: r_<field>[scenario, step]"""
    z["r_rewards_x2"], z["r_done"] = z["dl_r_rewards_x2"][:, None], z["dl_r_done"][:, None]


load = functools.partial(pins.load_npz, FIX_DIR, prepare=delivery_step_as_step_0)


def kwargs_of(task, **extra):
    env_id, over = rs.TASKS[task]
    return oracle_kwargs(env_id, **dict(over, **extra))


def scenarios_of(task):
    """The scenarios of a task rebuilt from its shape (not read from the fixture): (reset scenarios, delivery scenarios)."""
    m = load(task)["meta"]
    inc = rs.real_inc(m["seed"])
    return (rs.reset_scenarios(m["H"] * m["W"], m["N"], m["S"], m["Q"], inc),
            rs.delivery_scenarios(m["S"], m["Q"], m["N"], len(m["goals"]), inc))


# ------------------------------------------------------------------------------------------------------------------ numpy
def _bounded_three_ways(c):
    """One constructed state through numpy, the tracer and the oracle: (tracer record, 64-bit outputs consumed)."""
    n = c.n
    gen = rs.numpy_generator(c.state)
    want = int(gen.integers(0, n))
    want_end = rs.words_of_numpy(gen)
    t = rs.Tracer(c.state)
    got = t.bounded(n - 1)
    assert got == want and np.array_equal(t.words(), want_end), (c.name, n, "tracer", got, want, t.words(), want_end)
    st = c.state.copy()
    got = lib().orc_rng_bounded(st.ctypes.data, n - 1)
    assert got == want and np.array_equal(st, want_end), (c.name, n, "oracle", got, want, st, want_end)
    gen = rs.numpy_generator(c.state)        # the scalar `choice(candidates)` of the replacement request draws the same way
    assert int(gen.choice(np.arange(n))) == want and np.array_equal(rs.words_of_numpy(gen), want_end), (c.name, n, "choice(candidates)")
    return t.draws[-1], t.n64


@pytest.mark.parametrize("n", rs.BOUNDS + rs.POW2_BOUNDS)
def test_every_builder_matches_numpy_and_takes_the_branch_it_claims(n):
    cases = rs.bounded_cases(n, rs.real_inc(n))
    names = {c.name for c in cases}
    assert {"reject_buffered", "reject_low", "reject_both_halves", "reject_three", "leftover_in_if_no_loop", "leftover_eq_n", "value_0",
            "value_n_minus_1", "uinteger_all_ones", "rot_0", "rot_63", "pre_state_0", "pre_state_all_ones", "pre_state_lo_all_ones",
            "pre_state_hi_0"} <= names
    assert ({"leftover_eq_threshold", "leftover_below_threshold"} <= names) == (n not in rs.POW2_BOUNDS)
    for c in cases:
        assert int(c.state[3]) & 1, "numpy's increment is odd"
        d, n64 = _bounded_three_ways(c)
        if n in rs.POW2_BOUNDS:
            assert d.redraws == 0, (c.name, n, d)           # threshold == 0: no state may reject
        for what, claim, got in (("redraws", c.redraws, d.redraws), ("entered", c.entered, d.entered), ("value", c.value, d.value), ("n64", c.n64, n64)):
            assert claim is None or claim == got, f"n = {n}, {c.name}: claims {what} {claim}, the tracer found {got} ({d})"
    # the boundary states sit where they claim: leftover == threshold is the smallest accepted one, one granule below it is rejected
    thr, g = rs.threshold(n), rs.granule(n)
    if thr:
        for c in cases:
            lo = int(rs.output(rs.step(*rs.unwords(c.state)[:2]))) & 0xFFFFFFFF
            if c.name == "leftover_eq_threshold":
                assert (lo * n) & 0xFFFFFFFF == thr
            if c.name == "leftover_below_threshold":
                assert (lo * n) & 0xFFFFFFFF == thr - g and (g == 1) == bool(n & 1)


def test_a_bound_of_one_consumes_nothing_and_keeps_the_buffered_half():
    c = rs.n1_case(rs.real_inc(1))
    d, n64 = _bounded_three_ways(c)
    assert (d.value, d.redraws, n64) == (0, 0, 0)
    t = rs.Tracer(c.state)
    t.bounded(0)
    assert np.array_equal(t.words(), c.state) and int(c.state[4]) == 1


CHOICE_SHAPES = [(110, 2), (200, 4), (110, 4), (32, 2), (80, 4), (32, 8), (12, 3), (4, 3), (32, 3), (110, 9), (32, 9), (200, 16), (80, 16), (3, 3), (5, 5), (6, 5)]


@pytest.mark.parametrize("pop,k", CHOICE_SHAPES, ids=[f"{p}-{k}" for p, k in CHOICE_SHAPES])
def test_sampling_states_match_numpy_and_take_their_branch(pop, k):
    """choice(pop, k, replace=False): a Floyd collision (the `seen ? j : val` branch), a rejection in the Floyd pass and one in the
    Fisher-Yates pass — the shapes are the (HW, N) and (S, Q) of the fixture's tasks and three with pop == k (Floyd's j == 0)."""
    cases = rs.choice_cases(pop, k, rs.real_inc(pop + k))
    assert "floyd_collision" in {c.name for c in cases}
    assert ("fisher_yates_rejection" in {c.name for c in cases}) == any(rs.threshold(b) for b in range(2, k + 1))
    for c in cases:
        vals, end = rs.check_choice_claim(c)
        if c.name == "floyd_collision":
            assert pop - k + 1 in vals
        gen = rs.numpy_generator(c.state)
        want = gen.choice(pop, size=k, replace=False)
        want_end = rs.words_of_numpy(gen)
        assert list(want) == vals and np.array_equal(end, want_end), (c.name, pop, k, "tracer", vals, list(want))
        out, st = np.zeros(k, np.int32), c.state.copy()
        lib().orc_rng_choice(st.ctypes.data, pop, k, out.ctypes.data)
        assert list(want) == list(out) and np.array_equal(st, want_end), (c.name, pop, k, "oracle", list(out), list(want))


# ------------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_directory_stays_small():
    pins.check_fixture_directory_is_small(FIX_DIR, TASKS, limit=1_000_000)


@pytest.mark.parametrize("task", TASKS)
def test_fixture_holds_the_constructed_states_and_the_tracer_predicts_the_reference(task):
    """Per task: the fixture's states are the builders' (rebuilt here from the task's shape), every scenario takes the branch it claims,
    and the tracer — numpy's draws in Python integers, pinned against numpy above — predicts what the reference recorded: cells,
    directions, queue and state words after reset(); queue and state words after the delivery step."""
    z = load(task)
    m = z["meta"]
    HW, N, S, Q, W = m["H"] * m["W"], m["N"], m["S"], m["Q"], m["W"]
    resets, deliveries = scenarios_of(task)
    assert [sc.name for sc in resets] == m["reset_names"] and [sc.claim for sc in resets] == m["reset_claims"]
    assert [sc.name for sc in deliveries] == m["delivery_names"] and [sc.claim for sc in deliveries] == m["delivery_claims"]
    assert (len(resets), len(deliveries)) == (m["n_reset"], m["n_delivery"]) == (len(z["rs_rng0"]), len(z["dl_rng0"]))
    for k, sc in enumerate(resets):
        who = f"{task}, reset scenario {k} ({sc.name}, claims {sc.claim})"
        assert np.array_equal(sc.state, z["rs_rng0"][k]), who
        cells, dirs, queue, end = rs.check_reset_claim(sc, HW, N, S, Q)
        assert [c % W for c in cells] == z["rs_r_agent_x"][k].tolist() and [c // W for c in cells] == z["rs_r_agent_y"][k].tolist(), who
        assert dirs == z["rs_r_agent_dir"][k].tolist() and queue == z["rs_r_queue"][k].tolist() and np.array_equal(end, z["rs_r_rng"][k]), who
    for k, sc in enumerate(deliveries):
        who = f"{task}, delivery scenario {k} ({sc.name}, claims {sc.claim})"
        assert np.array_equal(sc.state, z["dl_rng0"][k]) and sc.queue == z["dl_queue"][k].tolist() and sc.on_goal == z["dl_on_goal"][k].tolist(), who
        queue, end = rs.check_delivery_claim(sc, S, Q)
        assert queue == z["dl_r_queue"][k].tolist() and np.array_equal(end, z["dl_r_rng"][k]), who
    names = set(m["reset_names"])
    need = {"cell_first_value_max", "cell_first_value_0", "cell_floyd_collision", "direction_takes_zero", "queue_first_value_max"}
    if rs.threshold(HW - N + 1):
        need |= {"cell_first_rejects_low", "cell_first_rejects_buffered", "cell_first_rejects_three", "cell_first_leftover_eq_threshold",
                 "cell_first_leftover_below_threshold"}
    if any(rs.threshold(b) for b in range(S - Q + 1, S + 1)):
        need |= {"queue_first_rejects", "queue_last_rejects"}
    assert need <= names, (task, sorted(need - names))
    n = S - Q
    dn = set(m["delivery_names"])
    for idx in {0, n - 1}:
        assert {f"idx_{idx}_{p}_{w}" for p in ("lowest", "highest") for w in ("smallest", "largest")} <= dn, (task, idx)
    assert {"two_goals_fresh_then_buffered", "two_goals_buffered_then_fresh"} <= dn
    if rs.threshold(n):
        assert {"draw_reject_buffered", "draw_reject_low", "draw_reject_both_halves", "draw_reject_three", "two_goals_second_rejects_buffered"} <= dn
        assert m["deliveries_with_rejection"] >= 7
    if n == 1:
        assert "one_candidate_keeps_buffer" in dn
    assert all(c > 0 for c in m["delivery_who"].values()), m["delivery_who"]
    # rewards[-1]: with nobody on the goal the last agent is paid (INDIVIDUAL, TWO_STAGE); GLOBAL pays everyone
    for k, sc in enumerate(deliveries):
        nd = sum(1 for s in sc.on_goal if s)
        if m["reward_type"] == 0:
            assert z["dl_r_rewards_x2"][k].tolist() == [2 * nd] * N
        elif sc.who == "nobody":
            assert z["dl_r_rewards_x2"][k].tolist() == [0] * (N - 1) + [nd * (2 if m["reward_type"] == 1 else 1)], (task, k)


def test_the_three_reward_types_and_a_single_candidate_are_in_the_fixture():
    assert {load(t)["meta"]["reward_type"] for t in TASKS} == {0, 1, 2}
    assert load("one-candidate")["meta"]["S"] - load("one-candidate")["meta"]["Q"] == 1 and len(load("one-candidate")["meta"]["goals"]) == 2
    n = load("prime-candidates")["meta"]["S"] - load("prime-candidates")["meta"]["Q"]
    assert all(n % d for d in range(2, n))


@pytest.mark.skipif(not rr.reference_available(), reason="/root/reference not present")
@pytest.mark.parametrize("task", ["tiny-2ag", "one-candidate", "prime-candidates"])
def test_reference_regenerates_the_committed_fixture(task, tmp_path):
    gen = pins.load_generator(os.path.join(FIX_DIR, "generate_rng_edges.py"))
    pins.assert_regenerates(gen.record_task(task, str(tmp_path)), os.path.join(FIX_DIR, f"{task}.npz"))


# ------------------------------------------------------------------------------------------------------------------ replay
RESET_FIELDS = ("agent_x", "agent_y", "agent_dir", "queue", "rng")
DELIVERY_FIELDS = ("queue", "agent_delivered", "rng")


def name_of(task, z, kind, k):
    m = z["meta"]
    return f"{task}, {kind} scenario {k} ({m[kind + '_names'][k]}, claims {m[kind + '_claims'][k]})"


def check_fields(task, z, kind, idx, state, fields, who, rew=None, done=None):
    pre = "rs_r_" if kind == "reset" else "dl_r_"
    for f in fields:
        got, want = np.asarray(state[f]), z[pre + f][idx]
        if not np.array_equal(got, want):
            bad = np.argwhere((got != want).reshape(len(idx), -1))[0]
            e, i = int(bad[0]), int(bad[1])
            raise AssertionError(f"{who}{name_of(task, z, kind, int(idx[e]))}: {f}[{i}] = {got[e].reshape(-1)[i]}, reference "
                                 f"{want[e].reshape(-1)[i]} (whole field {got[e].tolist()}, reference {want[e].tolist()})")
    pins.check_rewards(task, z, idx, 0, rew, done, who, name_of=lambda task, z, k, t: name_of(task, z, kind, k))


def delivery_fields(z, idx, rng=None, **extra):
    B, N = len(idx), z["meta"]["N"]
    f = {k: z["dl_" + k][idx].astype(np.int32) for k in ("agent_x", "agent_y", "agent_dir", "agent_carry", "queue")}
    f.update(agent_delivered=np.zeros((B, N), np.int32), steps=np.zeros(B, np.int32), inactive=np.zeros(B, np.int32),
             rng=z["dl_rng0"][idx] if rng is None else rng)
    f.update(extra)
    return f, np.ascontiguousarray(z["dl_shelf_xy"][idx].astype(np.int32))


def inject_delivery(be, z, idx, **extra):
    return pins.write_state(be, *delivery_fields(z, idx, **extra))


def oracle_run(task, z, ir, idl):
    """The oracle over reset scenarios `ir` and delivery scenarios `idl` (equally long), every recorded field against the fixture:
    returns what an engine is compared with beyond the fixture — (reset obs, reset state, injected obs, step obs, rewards, done, state)."""
    seed = z["meta"]["seed"]
    orc = OracleVecEnv(len(ir), **kwargs_of(task))
    orc.reset(seed=seed)
    orc.set_state(rng=z["rs_rng0"][ir])
    o_reset = orc.reset()
    s_reset = orc.get_state()
    check_fields(task, z, "reset", ir, s_reset, RESET_FIELDS, "oracle: ")
    o_inj = inject_delivery(orc, z, idl)
    rew, done = orc.step(np.zeros((len(idl), z["meta"]["N"]), np.int32))
    st = orc.get_state()
    check_fields(task, z, "delivery", idl, st, DELIVERY_FIELDS, "oracle: ", rew, done)
    return o_reset, s_reset, o_inj, orc.obs(), rew, done, st


def engine_run(task, z, ir, idl, who, library=None, rollout=False, **ctor):
    """One engine over the same batch: reset scenarios through reset(seed=None) (rw_reset with seeds = NULL), delivery scenarios through
    step() or a one-step rollout(); fixture and oracle, every field."""
    o_reset, s_reset, o_inj, o_step, rew2, done2, st2 = oracle_run(task, z, ir, idl)
    N = z["meta"]["N"]
    env = rware_amd.WarehouseVecEnv(len(ir), autoreset_mode="disabled", library=library, **kwargs_of(task), **ctor)
    try:
        env.reset(seed=z["meta"]["seed"])
        env.set_state(refresh_obs=False, rng=z["rs_rng0"][ir])
        obs, _ = env.reset(seed=None)
        st = env.get_state()
        check_fields(task, z, "reset", ir, st, RESET_FIELDS, who)
        same_state(st, s_reset, "reset")
        same_obs(obs, o_reset, "reset obs", "reset")
        same_obs(inject_delivery(env, z, idl), o_inj, "obs of the injected delivery state", "inject")
        a = np.zeros((len(idl), N), np.int32)
        if rollout:
            tape, rew, term = env.rollout(a[None])
            obs, rew, term = tape[0], rew[0], term[0]
        else:
            obs, rew, term, trunc, _ = env.step(a)
            assert not np.asarray(trunc).any()
        st = env.get_state()
        check_fields(task, z, "delivery", idl, st, DELIVERY_FIELDS, who, rew, term)
        same_state(st, st2, "delivery step")
        same_obs(obs, o_step, "obs after the delivery step", 0)
        assert np.array_equal(rew, rew2) and np.array_equal(np.asarray(term).astype(bool), done2.astype(bool))
        return env.engines[0].info
    finally:
        env.close()


def batch(z, multiple, ragged=False):
    """(reset scenario per env, delivery scenario per env): all of both, shuffled with a fixed seed, padded with copies of scenario 0
    to a whole number of `multiple` envs — or, `ragged`, to one env more: a partial last workgroup."""
    nr, nd = z["meta"]["n_reset"], z["meta"]["n_delivery"]
    g = np.random.default_rng(13)
    pad = lambda n: pins.pad_batch(np.concatenate([g.permutation(n), np.zeros(max(nr, nd) - n, np.int64)]), multiple, ragged)  # noqa: E731
    return pad(nr), pad(nd)


@pytest.mark.parametrize("task", TASKS)
def test_oracle_matches_reference_fixture(task):
    z = load(task)
    nr, nd = z["meta"]["n_reset"], z["meta"]["n_delivery"]
    B = max(nr, nd)
    oracle_run(task, z, np.arange(B) % nr, np.arange(B) % nd)


@pytest.mark.parametrize("task,build,rollout", [
    ("tiny-2ag", "generic", False), ("small-4ag", "generic", False), ("tiny-4ag-easy", "generic", False), ("one-candidate", "generic", False),
    ("prime-candidates", "generic", False), ("tiny-9ag", "generic", False),
    ("small-4ag", "static", False), ("small-4ag", "static", True), ("tiny-9ag", "static", False)])
def test_emulated_engine_matches_reference_fixture(task, build, rollout):
    """The product's rware_pcg64.h, reset and goal phases on host threads: the generic kernel with a partial last workgroup, and
    ahead-of-time builds (per-step launch and one-step rollout; 9 agents: the agent phase in LDS)."""
    z = load(task)
    ir, idl = batch(z, 4, ragged=True) if build == "generic" else batch(z, 16)
    assert len(ir) <= 112
    geom = dict(envs_per_workgroup=4, threads_per_workgroup=64) if build == "generic" else {}
    info = engine_run(task, z, ir, idl, f"emulated {build} kernel: ", library=emu_library(), rollout=rollout, **geom)
    assert (info.build_kind == 0) == (build == "generic")


@pytest.mark.parametrize("backend", ["emulated", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("task", ["tiny-2ag", "small-4ag"])
def test_reset_from_every_builder_state_matches_the_oracle(task, backend):
    """One constructed state per env — every builder at the bound of the first cell draw, the sampling states of the cell draws and
    the scenario states of the fixture —, shuffled, written with set_state(rng=...), then reset(seed=None): every state field and the
    observation against the oracle (pinned on numpy and on the fixture above).  Generic kernel, partial last workgroup."""
    m = load(task)["meta"]
    HW, N = m["H"] * m["W"], m["N"]
    inc = rs.real_inc(m["seed"])
    states = [c.state for c in rs.bounded_cases(HW - N + 1, inc)] + [c.state for c in rs.choice_cases(HW, N, inc)] + list(load(task)["rs_rng0"])
    states = np.stack(states)[np.random.default_rng(3).permutation(len(states))]
    states = np.concatenate([states, np.repeat(states[:1], (-len(states)) % 4 + 1, 0)])
    B = len(states)
    assert B % 4 == 1 and B <= 112
    library = None
    if backend == "emulated":
        library = emu_library()
    orc = OracleVecEnv(B, **kwargs_of(task))
    env = rware_amd.WarehouseVecEnv(B, autoreset_mode="disabled", library=library, envs_per_workgroup=4, threads_per_workgroup=64, **kwargs_of(task))
    try:
        env.reset(seed=1)
        orc.reset(seed=1)
        env.set_state(refresh_obs=False, rng=states)
        orc.set_state(rng=states)
        same_obs(env.reset(seed=None)[0], orc.reset(), "reset obs", "reset")
        same_state(env.get_state(), orc.get_state(), "reset")
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------------------ autoreset
def autoreset_batch(task, z, B):
    """Delivery scenarios whose step also ends the episode (steps = max_steps - 1 written beforehand).  Env 0 .. 3 carry states built
    for the pair of draws: the delivery takes the low half and leaves a buffered half that the first reset draw (bound HW - N + 1)
    rejects — once, or together with the next low half.  The claim is checked here with the tracer."""
    m = z["meta"]
    HW, N, S, Q = m["H"] * m["W"], m["N"], m["S"], m["Q"]
    n, n0 = S - Q, HW - N + 1
    inc = rs.real_inc(m["seed"])
    idl = np.arange(B) % m["n_delivery"]
    idl[:4] = 0                                     # (scenario 0: one delivery)
    rng = z["dl_rng0"][idl].copy()
    assert sum(1 for s in z["dl_on_goal"][0] if s) == 1 and rs.threshold(n0)
    lo = rs.accepted_value(n, n // 2) if n > 1 else 7
    for e in range(4):
        if n > 1 and e < 2:       # fresh low half to the delivery, the buffered high half is rejected by the reset
            rng[e] = rs._state(inc, 0, 0, lo, rs.rejected_value(n0, e))
        elif n > 1:               # buffered half to the delivery; the reset rejects both halves of the fresh output
            rng[e] = rs._state(inc, 1, lo, rs.rejected_value(n0, e), rs.rejected_value(n0, 1))
        else:                                       # S - Q == 1: the delivery consumes nothing, the buffered half goes to the reset as it is
            rng[e] = rs._state(inc, 1, rs.rejected_value(n0, e), rs.rejected_value(n0, e + 1), rs.SAFE)
        t = rs.Tracer(rng[e])
        t.bounded(n - 1)
        t.reset(HW, N, S, Q)
        # (at least: the value behind the last chosen one is the next 64-bit output, which inversion does not choose; S - Q == 1
        #  chooses all three values — two rejected ones, then SAFE — and is exact)
        want = rs.AtLeast(1 if e < 2 else 2) if n > 1 else 2
        assert t.draws[0].redraws == 0 and rs.redraws_as_claimed(t.draws[1].redraws, want), (task, e, t.draws[:2])
    return idl, rng


def autoreset_run(task, mode, library=None, B=64, **ctor):
    z = load(task)
    kw = kwargs_of(task)
    idl, rng = autoreset_batch(task, z, B)
    steps = np.full(B, kw["max_steps"] - 1, np.int32)
    orc = OracleVecEnv(B, **kw)
    env = rware_amd.WarehouseVecEnv(B, autoreset_mode=mode, library=library, **kw, **ctor)
    try:
        same_obs(env.reset(seed=z["meta"]["seed"])[0], orc.reset(seed=z["meta"]["seed"]), "reset obs", "reset")
        same_obs(inject_delivery(env, z, idl, rng=rng, steps=steps), inject_delivery(orc, z, idl, rng=rng, steps=steps), "injected obs", "inject")
        a = np.zeros((2, B, z["meta"]["N"]), np.int32)
        run = lockstep(env, orc, a[:1] if mode == "same_step" else a, mode, seed=None, state_every=1)
        assert run.episodes == B and run.finals == (B if mode == "same_step" else 0)
        return env.engines[0].info
    finally:
        env.close()


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("task", ["tiny-2ag", "one-candidate"])
def test_emulated_delivery_draw_and_reset_draws_share_one_stream(task, mode):
    """The terminating step draws the replacement request and (same_step: in the same launch; next_step: in the next one) the reset
    draws, from a state in which the delivery leaves a buffered half that the first reset draw rejects; the terminal observation
    (RW_BUF_FINAL_OBS) is compared too.  The oracle is the reference here: it is pinned on the fixture above."""
    autoreset_run(task, mode, library=emu_library(), B=17, envs_per_workgroup=4, threads_per_workgroup=64)


# ------------------------------------------------------------------------------------------------------------------ Q >= S
FOUR_SHELVES = ".xx.\n.xx.\n.gg."


def _engine(q, library=None):
    """rw_create itself, under WarehouseVecEnv: one engine of 4 envs on the 4-shelf layout."""
    from rware_amd.layout import layout_from_str
    return rware_amd._capi.Engine(num_envs=4, layout=layout_from_str(FOUR_SHELVES), n_agents=2, sensor_range=1, request_queue_size=q,
                                  max_inactivity_steps=0, max_steps=500, reward_type=1, autoreset_mode="disabled", library=library)


def rw_create_refuses(library=None):
    """rw_create returns RW_ERR_INVALID_ARG for Q == S and Q == S + 1, and its message says what the reference does there and where
    (ValueError at the first delivery: choice([]), rware/warehouse.py:915-916).  No engine exists afterwards: nothing was launched."""
    for q in (4, 5):
        with pytest.raises(rware_amd._capi.EngineError, match=rf"request_queue_size {q} >= shelves 4") as ei:
            _engine(q, library)
        assert ei.value.code == rware_amd._capi.RW_ERR_INVALID_ARG
        assert "ValueError at its first delivery" in str(ei.value) and "rware/warehouse.py:915-916" in str(ei.value)


def test_emulated_rw_create_refuses_a_request_queue_as_large_as_the_shelf_count():
    """The library's own check, reached through _capi.Engine (what bench.py and rw_multi users build).  Q == 0 and Q == S - 1 stay
    valid and reset."""
    rw_create_refuses(emu_library())
    for q in (0, 3):
        eng = _engine(q, emu_library())
        eng.reset(np.arange(4))
        assert eng.read("queue").shape == (4, q)
        eng.close()


def test_env_and_oracle_refuse_a_request_queue_as_large_as_the_shelf_count():
    """WarehouseVecEnv and the oracle raise ValueError at construction, in front of any engine (pure Python: `library` is never
    loaded); Q == 0 and Q == S - 1 stay valid."""
    for q in (4, 5):
        with pytest.raises(ValueError, match="request_queue_size"):
            rware_amd.WarehouseVecEnv(4, layout=FOUR_SHELVES, n_agents=2, request_queue_size=q, library="/nonexistent/library.so")
        with pytest.raises(ValueError, match="request_queue_size"):
            OracleVecEnv(4, layout=FOUR_SHELVES, n_agents=2, request_queue_size=q)
    for q in (0, 3):
        OracleVecEnv(4, layout=FOUR_SHELVES, n_agents=2, request_queue_size=q).reset(seed=1)


@pytest.mark.gpu
def test_gpu_rw_create_refuses_a_request_queue_as_large_as_the_shelf_count():
    """The device library's rw_create: create only — the refusal comes from the config check, before a device is touched or a kernel
    launched."""
    rw_create_refuses()


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("rollout", [False, True], ids=["step", "rollout"])
@pytest.mark.parametrize("task", TASKS)
def test_gpu_ahead_of_time_build_matches_reference_fixture(task, rollout):
    """The library's choice at its default geometry: an ahead-of-time build for the registered tasks (9 and 16 agents: the agent phase
    in LDS), whatever it picks for the two custom shapes."""
    z = load(task)
    info = engine_run(task, z, *batch(z, 32), "ahead-of-time build: ", rollout=rollout)
    assert info.jit == 0 and (info.build_kind in (1, 2) or task not in REGISTERED), (info.build_kind, info.jit)


@pytest.mark.gpu
@pytest.mark.parametrize("rollout", [False, True], ids=["step", "rollout"])
@pytest.mark.parametrize("task", TASKS)
def test_gpu_generic_kernel_matches_reference_fixture(task, rollout):
    z = load(task)
    ir, idl = batch(z, 4, ragged=True)
    assert len(ir) % 4 == 1
    info = engine_run(task, z, ir, idl, "generic kernel: ", rollout=rollout, envs_per_workgroup=4, threads_per_workgroup=64)
    assert info.build_kind == 0 and info.jit == 0 and info.envs_per_workgroup == 4


@pytest.mark.gpu
def test_gpu_runtime_build_matches_reference_fixture(tmp_path, monkeypatch):
    """rware_pcg64.h once more through hipRTC."""
    monkeypatch.setenv("RWARE_JIT_CACHE", str(tmp_path))
    z = load("prime-candidates")
    for rollout in (False, True):
        info = engine_run("prime-candidates", z, *batch(z, 32), "run-time exact-shape build: ", rollout=rollout, jit="force")
        assert info.build_kind == 1 and info.jit in (1, 2), (info.build_kind, info.jit)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("task,geom", [("tiny-2ag", {}), ("small-4ag", {}), ("one-candidate", dict(envs_per_workgroup=4, threads_per_workgroup=64)),
                                       ("tiny-9ag", {})], ids=["tiny-2ag", "small-4ag", "one-candidate-generic", "tiny-9ag"])
def test_gpu_delivery_draw_and_reset_draws_share_one_stream(task, geom, mode):
    info = autoreset_run(task, mode, B=65 if geom else 64, **geom)
    assert (info.build_kind == 0) == bool(geom)
