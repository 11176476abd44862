"""Warehouses of 65 .. 127 agents: the generic kernel's two-agents-per-lane agent phases (rware_phase_agents_wide.h).

The C oracle stops at 64 agents, so every engine here is checked against fixtures recorded from the reference itself
(tests/golden/wide/, tests/wide_fixtures.py): four random traces and one scripted one, and constructed states whose chains, cycles
and contested cells cross agent index 64 — the boundary between the two agents a lane owns.

  - CPU suite: the product sources on host threads (tests/emu), where the threads of a wavefront are NOT in lockstep — a sub-phase
    that reads what another agent's same sub-phase writes fails there.  The traces are replayed up to a dozen steps behind their
    first reset.
  - GPU suite (-m gpu): the same checks on the gfx950 library, every trace in full, plus a captured graph.
Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import collision_scenarios as cs
import golden_util as gu
import pins
import wide_fixtures as wf
from device_backends import BACKENDS, Gpu
from engine_backend import EngineBackend
from models import PLAIN, EpisodeModel, mask_model, same_buffers, same_everything

import rware_amd
from rware_amd import _capi
from rware_amd.vector_env import global_image_from_state

GEOMS = [(4, 256), (4, 64)]                 # one env per wavefront / one wavefront walks all four envs
GEOM_IDS = ["e4t256", "e4t64"]
MODES = ["next_step", "same_step", "disabled"]
ALL_TRACES = wf.TRACES + wf.SCRIPTED
TILE = 3                                    # 2 envs x 3 = 6: the second 4-env workgroup is ragged
OPT_IN = dict(stats=True, episode_stats=True, action_mask=True, time_limit_truncates=True)


def is_gpu(backend):
    return backend is Gpu


def steps_of(backend, meta):
    """GPU: the whole trace.  Host threads: its first reset and a dozen steps of the next episode."""
    return meta["T"] if is_gpu(backend) else min(meta["T"], meta["kwargs"]["max_steps"] + 12)


def make_env(backend, kw, B, geom=(0, 0), **more):
    return rware_amd.WarehouseVecEnv(B, library=backend.library(), envs_per_workgroup=geom[0], threads_per_workgroup=geom[1],
                                     **dict(kw, **more))


def tiled(a, axis):
    return np.concatenate([a] * TILE, axis=axis)


def image_of(obs):
    return obs["image"] if isinstance(obs, dict) else obs


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())


# ------------------------------------------------------------------------------------------------ the fixtures themselves (CPU)
def test_fixtures_are_small_and_every_trace_resets_twice_and_crosses_the_slot_boundary():
    for name in ALL_TRACES + (wf.STRADDLE,):
        assert os.path.getsize(os.path.join(wf.WIDE_DIR, name + ".npz")) < 512 * 1024, name
    for name in wf.TRACES:
        meta, z = wf.load_trace(name)
        assert meta["kwargs"]["n_agents"] > wf.SLOT and meta["E"] == 2 and 120 <= meta["T"] <= 200
        assert z["was_reset"].sum(0).min() >= 2, name
        found = wf.trace_straddles(z, z["grid"].shape[-1])
        assert found and all(min(c) < wf.SLOT <= max(c) and len(c) >= 2 for _, _, c in found), name
    meta, z = wf.load_trace(wf.SCRIPTED[0])
    assert meta["kwargs"]["reward_type"] == 0 and (z["rewards"] > 0).all(-1).any(), "no GLOBAL reward was ever paid"


# scenario -> (classes its step-0 move graph must hold, agents that must move, agents that must stay)
STRADDLE_WANT = {
    "chain-62-65": ("chain_3", {62, 63, 64, 65}, set()),
    "cycle-62-65": ("cycle_4", {62, 63, 64, 65}, set()),
    "swap-0-64": ("swap", set(), {0, 64}),
    "tie-3-70": ("junction_tie", {3}, {70}),
    "deeper-70-3": ("junction_unequal", {70, 71}, {3}),
    "blocked-64": ("chain_blocked_stationary", set(), {63, 64, 65}),
    "cancelled-100": ("chain_blocked_shelf", set(), {99, 100}),
    "loaded-100-127": ("loaded_follows_loaded+chain_1", {100, 126}, set()),
    "delivers-127": ("chain_0", {126}, set()),
}


def test_constructed_states_hold_every_class_across_the_slot_boundary():
    z = wf.load_straddle()
    H, W, N = z["meta"]["H"], z["meta"]["W"], z["meta"]["N"]
    assert N == 127 and sorted(z["variant"].tolist()) == sorted(STRADDLE_WANT)
    for k, variant in enumerate(z["variant"].tolist()):
        claim, move, stay = STRADDLE_WANT[variant]
        st = {f: z[f][k] for f in ("agent_x", "agent_y", "agent_dir", "agent_carry")}
        layer = cs.shelf_layer_from_xy(z["shelf_xy"][k], H, W)
        census, movers = cs.analyse(st["agent_x"], st["agent_y"], st["agent_dir"], st["agent_carry"], z["actions"][k, 0], H, W, layer)
        assert cs.class_matches(cs.census(st, z["actions"][k, 0], H, W, layer), claim) and str(z["claim"][k]) == claim, (variant, dict(census))
        assert move <= movers and not (stay & movers), (variant, sorted(movers))
        # ... and that is what the reference did
        moved = set(np.flatnonzero((z["r_agent_x"][k, 0] != z["agent_x"][k]) | (z["r_agent_y"][k, 0] != z["agent_y"][k])).tolist())
        assert moved == movers, (variant, sorted(moved ^ movers))
        if variant not in ("cancelled-100", "loaded-100-127", "delivers-127"):   # (those sit in the second slot: the loaded-agent rules there)
            assert min(move | stay) < wf.SLOT <= max(move | stay), variant
    k = z["variant"].tolist().index("loaded-100-127")
    assert z["agent_carry"][k, 126] > 0 and z["agent_carry"][k, 100] > 0       # the last id, loaded: agent-layer byte 0xFF
    k = z["variant"].tolist().index("delivers-127")
    assert z["r_rewards_x2"][k, 0, 126] == 1 and z["r_agent_delivered"][k, 0, 126] == 1


# ------------------------------------------------------------------------------------------------ traces, step by step
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("name", ALL_TRACES)
def test_generic_kernel_replays_the_references_trace(name, geom, backend):
    meta, z = wf.load_trace(name)
    be = EngineBackend(meta["E"], library=backend.library(), tile=TILE, jit="off", envs_per_workgroup=geom[0], threads_per_workgroup=geom[1],
                       **gu.ctor_kwargs(meta))
    try:
        info = be.env.engines[0].info
        assert (info.build_kind, info.specialised, info.envs_per_workgroup, info.threads_per_workgroup) == (0, 0) + geom
        assert gu.replay(be, meta, z, steps=steps_of(backend, meta)) > meta["kwargs"]["max_steps"]
        if name == "small-127ag-twostage":   # behind the last step: the critic's image, built on the device from the kernels' own state
            st = be.env.get_state()
            for layers in (PLAIN, [1, 2]):
                got = be.env.global_image_device(layers)
                same(got, global_image_from_state(st, be.env.goals, layers), ("global image", layers))
    finally:
        be.env.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_constructed_states_step_like_the_reference(geom, backend):
    """the nine scenarios as one batch (ragged: 4 + 4 + 1), four steps one by one, then the same four as one fused rollout"""
    z = wf.load_straddle()
    idx = np.arange(z["meta"]["n"])
    for fused in (False, True):
        pins.engine_run(wf.STRADDLE, z, idx, fused, "fused: " if fused else "", z["meta"]["kwargs"], pins.fixture_outputs(z, idx),
                        fields=pins.AGENT_FIELDS + ("shelf_xy", "queue", "rng"), name_of=cs.name_of, library=backend.library(),
                        envs_per_workgroup=geom[0], threads_per_workgroup=geom[1], jit="off")


# ------------------------------------------------------------------------------------------------ fused rollouts
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ALL_TRACES)
def test_fused_rollout_equals_the_per_step_outputs(name, mode, backend):
    """one launch over the trace's actions == the same steps one by one: the three tapes, the final state — in every autoreset mode,
    on the default geometry (4 envs per 256-thread workgroup)"""
    meta, z = wf.load_trace(name)
    kw, T = gu.ctor_kwargs(meta), steps_of(backend, meta)
    B = meta["E"] * TILE
    acts = tiled(z["actions"][:T].astype(np.int32), 1)
    a, b = (make_env(backend, kw, B, autoreset_mode=mode) for _ in range(2))
    try:
        info = a.engines[0].info
        assert (info.build_kind, info.envs_per_workgroup, info.threads_per_workgroup) == (0, 4, 256)
        seeds = np.tile(np.uint64(meta["seed"]) + np.arange(meta["E"], dtype=np.uint64), TILE)
        same(image_of(a.reset(seed=seeds)[0]), image_of(b.reset(seed=seeds)[0]), "reset")
        stepwise = [a.step(acts[t]) for t in range(T)]
        obs, rew, term = b.rollout(acts)
        for t, (o, r, d, _, _) in enumerate(stepwise):
            same(obs[t], image_of(o), ("observation tape", t))
            same(rew[t], r, ("reward tape", t))
            same(term[t], d, ("terminated tape", t))
            if mode == "next_step":   # (and the per-step outputs are the reference's)
                same(r, tiled(z["rewards"][t], 0), ("reward", t))
                same(d, tiled(z["done"][t], 0).astype(bool), ("done", t))
        assert np.any([d.any() for _, _, d, _, _ in stepwise]), "no episode ended inside the rollout"
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            same(sb[k], sa[k], ("state behind the rollout", k))
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ N = 65, every opt-in output
@pytest.mark.parametrize("backend", BACKENDS)
def test_65_agents_with_every_opt_in_output(backend):
    meta, z = wf.load_trace("tiny-65ag")
    kw, T = gu.ctor_kwargs(meta), steps_of(backend, meta)
    B, N = meta["E"] * TILE, kw["n_agents"]
    seeds = np.tile(np.uint64(meta["seed"]) + np.arange(meta["E"], dtype=np.uint64), TILE)
    flt = make_env(backend, kw, B, GEOMS[1], jit="off", **OPT_IN)
    pk = make_env(backend, kw, B, GEOMS[0], jit="off", obs_format="packed", **OPT_IN)
    try:
        assert flt.engines[0].info.build_kind == 0 and pk.engines[0].info.obs_packed == 1
        model = EpisodeModel(B, N, "next_step")
        o_f, o_p = flt.reset(seed=seeds)[0], pk.reset(seed=seeds)[0]
        same(pk.unpack_obs(o_p), o_f, "reset: unpacked rows")
        same(o_f, tiled(z["obs0"], 0), "reset: rows")
        max_steps, max_inact = kw["max_steps"], kw["max_inactivity_steps"]
        for t in range(T):
            a = tiled(z["actions"][t].astype(np.int32), 0)
            o_f, r_f, term_f, trunc_f, _ = flt.step(a)
            o_p, r_p, term_p, trunc_p, _ = pk.step(a)
            same(pk.unpack_obs(o_p), o_f, ("unpacked rows", t))
            same(o_f, tiled(z["obs"][t].astype(np.float32), 0), ("rows", t))
            same(r_f, tiled(z["rewards"][t], 0), ("rewards", t))
            same(r_p, r_f, ("rewards of the packed twin", t))
            # the two ends of an episode, from the counters the reference held when it said `done`
            done = z["done"][t].astype(bool)
            want_trunc = done & bool(max_steps) & (z["steps"][t] >= (max_steps or 0))
            want_term = done & bool(max_inact) & (z["inactive"][t] >= (max_inact or 0))
            assert np.array_equal(want_trunc | want_term, done)
            for term, trunc in ((term_f, trunc_f), (term_p, trunc_p)):
                same(term, tiled(want_term, 0), ("terminated", t))
                same(trunc, tiled(want_trunc, 0), ("truncated", t))
            model.step(tiled(z["rewards"][t], 0), tiled(done, 0))
            for env in (flt, pk):
                same_buffers(env.episode_stats(), model, t)
                want_mask, _ = mask_model(env.get_state(), np.asarray(env.highways))
                same(env.engines[0].read("action_mask"), want_mask, ("action mask", t))
        assert model.v["count"].min() >= 1
        # INDIVIDUAL rewards: a delivery pays 1.0 to one agent, so the reference's rewards count the deliveries
        want_deliveries = tiled(z["rewards"][:T].sum((0, 2)), 0).astype(np.int64)
        for env in (flt, pk):
            same(np.asarray(env.event_counters()["deliveries"]).astype(np.int64), want_deliveries, "deliveries")
    finally:
        flt.close(); pk.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("obs_type", [2, 3], ids=["image", "image_dict"])
def test_uint8_images_are_the_float_images(obs_type, backend):
    meta, z = wf.load_trace("imgdict-medium-100ag-sr2")
    kw = dict(gu.ctor_kwargs(meta), observation_type=obs_type)
    B, T = meta["E"] * TILE, kw["max_steps"] + 3
    seeds = np.tile(np.uint64(meta["seed"]) + np.arange(meta["E"], dtype=np.uint64), TILE)
    flt, u8 = make_env(backend, kw, B, jit="off"), make_env(backend, kw, B, jit="off", obs_format="uint8")
    try:
        o_f, o_u = image_of(flt.reset(seed=seeds)[0]), image_of(u8.reset(seed=seeds)[0])
        assert o_u.dtype == np.uint8
        same(o_u, o_f.astype(np.uint8), "reset")
        for t in range(T):
            a = tiled(z["actions"][t].astype(np.int32), 0)
            o_f, o_u = image_of(flt.step(a)[0]), image_of(u8.step(a)[0])
            assert o_u.dtype == np.uint8
            same(o_u, o_f.astype(np.uint8), t)
            same(o_f, tiled(z["obs"][t], 0), ("the float image", t))   # (the image does not depend on the observation type's wrapper)
    finally:
        flt.close(); u8.close()


# ------------------------------------------------------------------------------------------------ the other launch forms
@pytest.mark.parametrize("backend", BACKENDS)
def test_snapshot_restore_and_masked_resets_from_host_and_device(backend):
    be = backend()
    meta, z = wf.load_trace("medium-96ag-msg1-global-inact")
    kw = gu.ctor_kwargs(meta)
    B = meta["E"] * TILE
    acts = tiled(z["actions"][:13].astype(np.int32), 1)
    a, b = (make_env(be, kw, B, autoreset_mode="disabled", **OPT_IN) for _ in range(2))
    try:
        for env in (a, b):
            env.reset(seed=7)
            for t in range(3):
                env.step(acts[t])
        # a snapshot, five steps, a restore, the same five steps
        snap = a.snapshot()
        first = [a.step(acts[t]) for t in range(3, 8)]
        a.restore(snap)
        second = [a.step(acts[t]) for t in range(3, 8)]
        for t, (x, y) in enumerate(zip(first, second)):
            for k in range(4):
                same(y[k], x[k], ("behind the restore", t, k))
        a.free_snapshot(snap)
        for t in range(3, 8):
            b.step(acts[t])
        # a masked reset with seeds: the host path on one twin, the device path (rw_reset_device) on the other
        seeds = (np.arange(B, dtype=np.uint64) * np.uint64(977) + np.uint64(5))
        mask = (np.arange(B) % 3 != 1).astype(np.uint8)
        a.reset(seed=seeds, mask=mask.astype(bool))
        b.engines[0].reset_device(be.ptr(seeds), be.ptr(mask))
        same_everything(a, b, "behind the masked resets")
        for t in range(8, 13):
            a.step(acts[t]); b.step(acts[t])
        same_everything(a, b, "five steps on")
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_step_tape_device_equals_stepwise_calls(backend):
    meta, z = wf.load_trace("tiny-65ag")
    kw = gu.ctor_kwargs(meta)
    B, TS = meta["E"] * TILE, 5
    a, b = (make_env(backend, kw, B) for _ in range(2))
    try:
        a.reset(seed=11); b.reset(seed=11)
        tape = np.ascontiguousarray(tiled(z["actions"][:TS].astype(np.int32), 1))
        eng = a.engines[0]
        d = C.c_void_p()
        eng._check(eng.lib.rw_device_malloc(eng._h, tape.nbytes, C.byref(d)))
        eng._check(eng.lib.rw_copy_to_device(eng._h, d, tape.ctypes.data, tape.nbytes))
        eng.step_tape_device(d.value, TS, 3, 9)           # rows 3, 4, 0, 1, 2, 3, ...
        eng.sync()
        for k in range(9):
            obs, rew, _, _, _ = b.step(tape[(3 + k) % TS])
        same(a.observations(), obs, "observations")
        same(eng.read("rewards"), rew, "rewards")
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            same(sa[k], sb[k], k)
        eng.lib.rw_device_free(eng._h, d)
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_a_captured_graph_of_three_steps_equals_three_steps():
    import torch

    meta, z = wf.load_trace("small-127ag-twostage")
    kw = gu.ctor_kwargs(meta)
    B = 16
    acts = np.random.default_rng(3).choice(5, size=(B, kw["n_agents"]), p=[.05, .7, .1, .1, .05]).astype(np.int32)
    a = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
    b = rware_amd.WarehouseVecEnv(B, **kw)
    try:
        a.reset(seed=5); b.reset(seed=5)
        at = torch.from_numpy(acts).cuda()
        loop = a.capture_loop(lambda obs, rew, term: at, steps=3)
        loop.replay()
        a.sync()
        for _ in range(3):
            obs, rew, _, _, _ = b.step(acts)
        same(a.observations().cpu().numpy(), obs, "observations")
        sa, sb = a.get_state(), b.get_state()
        for k in sb:
            same(np.asarray(sa[k]), sb[k], k)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ construction
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_boundary_of_the_agent_count(backend):
    lib = backend.library()
    medium = dict(shelf_columns=5, column_height=8, shelf_rows=2, request_queue_size=40, max_steps=50)
    env = rware_amd.WarehouseVecEnv(5, library=lib, n_agents=127, **medium)
    info = env.engines[0].info
    assert (info.n_agents, info.build_kind, info.specialised, info.envs_per_workgroup, info.threads_per_workgroup) == (127, 0, 0, 4, 256)
    env.close()
    env = rware_amd.WarehouseVecEnv(16, library=lib, n_agents=127, envs_per_workgroup=16, **medium)   # 16 x 127 = 2032 agents per workgroup
    assert env.engines[0].info.envs_per_workgroup == 16
    env.close()
    with pytest.raises(_capi.EngineError, match=r"n_agents 128 not in 1\.\.127.*one byte.*wider layer") as err:
        rware_amd.WarehouseVecEnv(5, library=lib, n_agents=128, **medium)
    assert err.value.code == _capi.RW_ERR_INVALID_ARG
    with pytest.raises(_capi.EngineError, match=r"envs_per_workgroup 20 too large for N=124.*2355") as err:
        rware_amd.WarehouseVecEnv(20, library=lib, n_agents=124, envs_per_workgroup=20, **medium)
    assert err.value.code == _capi.RW_ERR_INVALID_ARG
    env = rware_amd.WarehouseVecEnv(8, library=lib, n_agents=65, jit="force", pipe=True, **medium)   # neither a run-time nor a pipelined build
    info = env.engines[0].info
    assert info.build_kind == 0 and info.specialised == 0 and info.pipe_workgroups == 0
    assert "more than 64 agents: the generic kernel" in env.engines[0].jit_log()
    env.reset(seed=1)
    env.step(np.ones((8, 65), np.int32))
    env.close()


def test_the_18_bit_reciprocal_is_exact_below_2355_agents_per_workgroup():
    """rw_div18(x, magic18(N)) == x // N for every x < 2355 and every N in 65 .. 127; 2355 / 124 is the first miss"""
    x = np.arange(4096, dtype=np.uint64)
    first_miss = {}
    for n in range(65, 128):
        magic = np.uint64(((1 << 18) + n - 1) // n)
        bad = np.flatnonzero(((x * magic) & np.uint64(0xFFFFFFFF)) >> np.uint64(18) != x // np.uint64(n))
        if len(bad):
            first_miss[n] = int(bad[0])
    assert min(first_miss.values()) == 2355 and first_miss[124] == 2355
