"""rw_snapshot_restore_indexed: single envs restored or cloned from a snapshot on the device, by index — the gather kernel,
Engine.restore_indexed, WarehouseVecEnv.restore(token, index=...) and clone_envs.

  - CPU suite: the product sources on host threads (tests/emu; a device pointer is a host pointer there, so numpy arrays serve as the
    "device" index arrays), the generic step kernel on 4-env workgroups.
  - GPU suite (-m gpu): the same checks on the gfx950 library, then the torch surface: tensor indices, clone_envs inside a captured loop
    (a host synchronisation inside the capture would fail it).
Expectations: an OracleVecEnv whose saved state (its FIELDS arrays, agent_msg, the pending NEXT_STEP resets, the event counters) is
rearranged with the same index in numpy (tests/restore_cases.py); no engine output is compared against another engine output.  Every
comparison is exact (array_equal).  The C oracle steps at most 64 agents: the 70-agent shape moves on by resets with other seeds and
written counters, which the oracle can do at any agent count."""
import ctypes as C

import numpy as np
import pytest

import lockstep
import restore_cases as rc
from device_backends import BACKENDS, GENERIC, Gpu, emu_library
from models import bits, mask_model, same_buffers
from rware_oracle import OracleVecEnv

import rware_amd
from rware_amd import _capi

RNG_FIELDS = 6


def make_pair(be, B, kw, env_only=None, big=False):
    """(env, oracle) of one configuration; `big`: the emulated build on 32-env workgroups (a thread per lane — fewer, larger ones)"""
    kw = lockstep.oracle_kwargs(None, **kw)
    geom = dict(be.kw, envs_per_workgroup=32) if be.kw and big else be.kw
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), **dict(kw, **geom), **(env_only or {}))
    return env, OracleVecEnv(B, **kw)


def move_on(env, orc, rng, steps, episodes=None):
    """both sides `steps` random steps further — beyond 64 agents: a reset with another seed and written counters instead"""
    if orc.N <= 64:
        rc.play(env, orc, rng, steps, episodes=episodes)
        return
    seed = int(rng.integers(1, 2**31))
    lockstep.same_obs(env.reset(seed=seed)[0], orc.reset(seed=seed), "reset obs")
    counters = dict(steps=rng.integers(0, 50, size=orc.B).astype(np.int32), inactive=rng.integers(0, 50, size=orc.B).astype(np.int32),
                    agent_delivered=rng.integers(0, 2, size=(orc.B, orc.N)).astype(np.int32))
    env.set_state(**counters)
    orc.set_state(**counters)


def reseed(env, orc, seed):
    """other RNG streams on both sides: random play alone draws only at a delivery or a reset"""
    env.seed(seed)
    orc.seed(seed)


def differs_everywhere(now, saved):
    """the current state and the saved one differ in every env, so a row copied to the wrong place or not at all shows"""
    return all((now["rng"][e] != saved["rng"][e]).any() and (now["steps"][e] != saved["steps"][e] or not np.array_equal(now["grid"][e], saved["grid"][e]))
               for e in range(len(now["rng"])))


# ------------------------------------------------------------------------------------------------ 1. the state, field by field
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", list(rc.SHAPES))
def test_every_field_of_a_restored_env_is_its_slot_and_of_the_others_what_it_was(shape, backend):
    be = backend()
    B, kw = rc.SHAPES[shape]
    env, orc = make_pair(be, B, dict(kw, max_steps=30), big=(B == 300))
    eng = env.engines[0]
    assert (eng.H, eng.W) == {"wide-4x16": (4, 16), "29x28-10ag": (29, 28)}.get(shape, (11, 10))
    assert (eng.S > 255) == (shape == "29x28-10ag") and eng.N == kw["n_agents"]
    lockstep.same_obs(env.reset(seed=5)[0], orc.reset(seed=5), "reset obs")
    rng = np.random.default_rng(3)
    move_on(env, orc, rng, 6)
    token, saved = env.snapshot(), rc.Saved(orc)
    for k, kind in enumerate(rc.PATTERNS):
        move_on(env, orc, rng, 3)
        reseed(env, orc, 1000 + 50 * k)
        assert differs_everywhere(orc.get_state(), saved.f), kind
        lockstep.same_state(env.get_state(), orc.get_state(), "before " + kind)
        index = rc.index_pattern(kind, B)
        eng.restore_indexed(token[0], be.ptr(index))
        env.sync()
        hit = rc.rearrange(orc, saved, index)
        assert hit.sum() == {"none": 0, "identity": B, "reversal": B, "one-slot": B}.get(kind, hit.sum()) and (kind != "random" or 0 < hit.sum() < B)
        lockstep.same_state(env.get_state(), orc.get_state(), kind)
        lockstep.same_obs(env.observations(), orc.obs(), "obs after " + kind)
    env.free_snapshot(token)
    env.close()


# ------------------------------------------------------------------------------------------------ 2. the RNG is copied whole
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_restored_streams_continue_and_a_pending_reset_travels_with_its_slot(backend):
    """max_steps 8 on staggered step counters: at the snapshot some slots have just ended (a pending NEXT_STEP reset), others are in
    mid-episode, and streams with and without a buffered 32-bit half (has_uint32) are among the sources — asserted on the oracle."""
    be = backend()
    B = 12
    env, orc = make_pair(be, B, dict(rc.TINY, max_steps=8))
    eng = env.engines[0]
    env.reset(seed=31)
    orc.reset(seed=31)
    stagger = (np.arange(B) % 4).astype(np.int32)
    env.set_state(steps=stagger, refresh_obs=False)
    orc.set_state(steps=stagger)
    certain_delivery(env, orc, envs=(1, 5, 8))           # a delivery's replacement draw leaves a buffered 32-bit half behind
    forward = np.tile(np.array([[1, 0]], np.int32), (B, 1))
    env.step(forward)
    orc.step_autoreset(forward, "next_step")
    rng = np.random.default_rng(8)
    rc.play(env, orc, rng, 5)
    token, saved = env.snapshot(), rc.Saved(orc)
    index = rc.index_pattern("random", B)
    src = index[index >= 0]
    assert set(saved.f["rng"][src, 4].tolist()) == {0, 1}, "both values of has_uint32 have to be among the source slots"
    pending = saved.f["_prev_done"].astype(bool)
    assert pending[src].any() and not pending[src].all(), "slots with and without a pending reset have to be among the sources"
    rc.play(env, orc, rng, 5)
    # a) the reset draws continue each restored stream: the whole state, all six RNG fields included, matches afterwards
    eng.restore_indexed(token[0], be.ptr(index))
    hit = rc.rearrange(orc, saved, index)
    lockstep.same_state(env.get_state(), orc.get_state(), "restored")
    lockstep.same_obs(env.reset(mask=hit)[0], orc.reset(mask=hit.astype(np.uint8)), "masked reset obs")
    orc._prev_done[hit] = 0                              # (a reset env has no reset pending)
    lockstep.same_state(env.get_state(), orc.get_state(), "reset after the restore")
    # b) restored once more, then 30 steps: a clone of a slot with a pending reset resets on its next step
    eng.restore_indexed(token[0], be.ptr(index))
    rc.rearrange(orc, saved, index)
    clones_pending = hit & pending[np.maximum(index, 0)]
    assert clones_pending.any()
    a = rng.choice(5, size=(B, 2), p=rc.P_ACT).astype(np.int32)
    obs, rew, term, _, _ = env.step(a)
    o2, r2, d2 = orc.step_autoreset(a, "next_step")
    lockstep.same_obs(obs, o2, "obs of the first step")
    st = env.get_state()
    assert not st["steps"][clones_pending].any() and not rew[clones_pending].any() and not term[clones_pending].any()
    lockstep.same_state(st, orc.get_state(), "first step")
    run = lockstep.lockstep(env, orc, lambda t: rng.choice(5, size=(B, 2), p=rc.P_ACT).astype(np.int32), "next_step", seed=None, steps=30,
                            state_every=1)
    assert run.episodes >= B
    env.free_snapshot(token)
    env.close()


# ------------------------------------------------------------------------------------------------ 3. keep_rng
@pytest.mark.parametrize("backend", BACKENDS)
def test_keep_rng_leaves_every_stream_alone(backend):
    be = backend()
    B = 9
    env, orc = make_pair(be, B, dict(rc.TINY, max_steps=30))
    env.reset(seed=2)
    orc.reset(seed=2)
    rng = np.random.default_rng(5)
    rc.play(env, orc, rng, 5)
    token, saved = env.snapshot(), rc.Saved(orc)
    rc.play(env, orc, rng, 4)
    reseed(env, orc, 77)
    before = orc.get_state()["rng"]
    assert differs_everywhere(orc.get_state(), saved.f)
    for kind in ("random", "one-slot"):
        index = rc.index_pattern(kind, B)
        env.engines[0].restore_indexed(token[0], be.ptr(index), keep_rng=True)
        rc.rearrange(orc, saved, index, keep_rng=True)
        got = env.get_state()
        assert got["rng"].shape == (B, RNG_FIELDS) and np.array_equal(got["rng"], before), kind
        lockstep.same_state(got, orc.get_state(), kind)
    env.free_snapshot(token)
    env.close()


def certain_delivery(env, orc, envs=(0,)):
    """both sides, in `envs`: agent 0 stands above the first goal, faces it and carries the shelf the queue asks for first; agent 1 waits
    in the corner"""
    gx, gy = orc.goals[0]
    st, sxy = orc.get_state(), orc.shelf_xy()
    for e in envs:
        shelf = int(st["queue"][e, 0])
        st["agent_x"][e], st["agent_y"][e], st["agent_dir"][e], st["agent_carry"][e] = (gx, 0), (gy - 1, 0), (1, 0), (shelf, 0)
        sxy[e, shelf - 1] = (gx, gy - 1)
    orc.set_state(**{k: st[k] for k in ("agent_x", "agent_y", "agent_dir", "agent_carry")})
    orc.recalc_grid(sxy)
    env.set_state(**orc.get_state())
    lockstep.same_state(env.get_state(), orc.get_state(), "constructed")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("keep_rng", [True, False])
def test_clones_of_one_slot_draw_apart_with_keep_rng_and_together_without(keep_rng, backend):
    be = backend()
    B = 6
    env, orc = make_pair(be, B, dict(rc.TINY, max_steps=30))
    env.reset(seed=40)
    orc.reset(seed=40)
    certain_delivery(env, orc)
    index = np.zeros(B, np.int32)
    saved = rc.Saved(orc)
    env.clone_envs(index, keep_rng=keep_rng)                 # every env becomes env 0 as it is now
    rc.rearrange(orc, saved, index, keep_rng=keep_rng)
    lockstep.same_state(env.get_state(), orc.get_state(), "cloned")
    a = np.tile(np.array([[1, 0]], np.int32), (B, 1))        # agent 0 FORWARD onto the goal: the delivery
    _, rew, _, _, _ = env.step(a)
    _, r2, _ = orc.step_autoreset(a, "next_step")
    assert (r2[:, 0] == 1).all() and np.array_equal(rew, r2)
    q = orc.get_state()["queue"]
    if keep_rng:
        assert len({tuple(row) for row in q.tolist()}) > 1, "the oracle's clones have to draw different replacements"
    else:
        assert (q == q[0]).all()
    lockstep.same_state(env.get_state(), orc.get_state(), "after the delivery")
    env.close()


# ------------------------------------------------------------------------------------------------ 4. formats and opt-in outputs
OPT_IN = dict(action_mask=True, episode_stats=True, stats=True)
IMAGE = rware_amd.ObservationType.IMAGE
FORMATS = {
    "flattened-float32": ({}, {}),
    "packed": ({}, dict(obs_format="packed")),
    "image-float32": (dict(observation_type=IMAGE), {}),
    "image-uint8": (dict(observation_type=IMAGE), dict(obs_format="uint8")),
    "image-dict": (dict(observation_type=rware_amd.ObservationType.IMAGE_DICT), {}),
}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_observations_masks_and_statistics_follow_the_restore(fmt, backend):
    be = backend()
    B = 10
    both, env_only = FORMATS[fmt]
    env, orc = make_pair(be, B, dict(rc.TINY, max_steps=7, **both), dict(env_only, **OPT_IN))
    ep = rc.episode_model(orc)
    env.reset(seed=11)
    orc.reset(seed=11)
    rng = np.random.default_rng(7)
    rc.play(env, orc, rng, 9, episodes=ep)
    token, saved = env.snapshot(), rc.Saved(orc, ep)
    rc.play(env, orc, rng, 9, episodes=ep)
    assert saved.f["stat_failed_moves"].any() and ep.v["count"].any() and not np.array_equal(saved.ep[0]["length"], ep.v["length"])
    index = rc.index_pattern("random", B)
    obs = env.restore(token, index=index)                    # a host index: checked, uploaded
    rc.rearrange(orc, saved, index, episodes=ep)
    lockstep.same_obs(env.unpack_obs(obs) if fmt == "packed" else obs, orc.obs(), "obs")
    want, _ = mask_model(orc.get_state(), orc.hw)
    assert np.array_equal(env.action_mask(), bits(want)) and np.array_equal(env.action_mask(permissive=True), bits(want, True))
    same_buffers(env.episode_stats(), ep, fmt)
    counters = env.event_counters()
    assert np.array_equal(counters["deliveries"], orc.stat_deliveries) and np.array_equal(counters["failed_moves"], orc.stat_failed_moves)
    lockstep.same_state(env.get_state(), {k: v for k, v in orc.get_state().items()}, fmt)
    env.free_snapshot(token)
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_sharded_env_takes_a_host_index_within_its_shards(backend):
    be = backend()
    B = 10
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1")
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), devices=[0, 0, 0], **dict(kw, **be.kw))
    orc = OracleVecEnv(B, **kw)
    assert env.shard_bounds == [(0, 4), (4, 7), (7, 10)]
    env.reset(seed=8)
    orc.reset(seed=8)
    rng = np.random.default_rng(4)
    rc.play(env, orc, rng, 5)
    token, saved = env.snapshot(), rc.Saved(orc)
    rc.play(env, orc, rng, 5)
    index = np.array([1, 0, -1, 2, 6, 6, 4, -1, 9, 8], np.int64)
    before = orc.get_state()
    for bad in ([5] + index[1:].tolist(), index[:-1].tolist() + [3], [B] + index[1:].tolist(), [-2] + index[1:].tolist(), index[:-1], index.astype(np.float32)):
        with pytest.raises(ValueError):
            env.restore(token, index=bad)
    lockstep.same_state(env.get_state(), before, "a refused call has done nothing")
    lockstep.same_obs(env.restore(token, index=index), (rc.rearrange(orc, saved, index), orc.obs())[1], "obs")
    lockstep.same_state(env.get_state(), orc.get_state(), "sharded")
    saved = rc.Saved(orc)
    lockstep.same_obs(env.clone_envs(index.tolist()), (rc.rearrange(orc, saved, index), orc.obs())[1], "obs of the clones")
    lockstep.same_state(env.get_state(), orc.get_state(), "sharded clones")
    env.free_snapshot(token)
    env.close()


# ------------------------------------------------------------------------------------------------ 5. arguments
def test_the_entry_point_checks_its_arguments():
    B = 6
    env = rware_amd.WarehouseVecEnv(B, library=emu_library(), **dict(rware_amd.env_kwargs("rware-tiny-2ag-v1"), **GENERIC))
    eng = env.engines[0]
    env.reset(seed=1)
    token = env.snapshot()
    env.step(np.ones((B, 2), np.int32))
    before = env.get_state()
    index = np.zeros(B + 1, np.int32)
    assert index.ctypes.data % 4 == 0
    ptr, snap = C.c_void_p(index.ctypes.data), token[0]
    call, inv = eng.lib.rw_snapshot_restore_indexed, _capi.RW_ERR_INVALID_ARG
    assert call(None, snap, ptr, 0) == inv and call(eng._h, None, ptr, 0) == inv and call(eng._h, snap, None, 0) == inv
    for odd in (1, 2, 3):
        assert call(eng._h, snap, C.c_void_p(index.ctypes.data + odd), 0) == inv
    assert "4-byte aligned" in eng.lib.rw_last_error(eng._h).decode()
    for flags in (2, 3, 4, -1, 1 << 30):
        assert call(eng._h, snap, ptr, flags) == inv
    with pytest.raises(_capi.EngineError):
        eng.restore_indexed(snap, 0)
    eng.sync()
    lockstep.same_state(env.get_state(), before, "a refused call has done nothing")
    with pytest.raises(ValueError):
        env.restore(token, keep_rng=True)                     # keep_rng belongs to an indexed restore
    assert call(eng._h, snap, C.c_void_p(index.ctypes.data + 4), 1) == _capi.RW_OK
    eng.sync()
    env.free_snapshot(token)
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_an_index_out_of_range_keeps_its_env_and_shows_at_the_next_sync(backend):
    """the kernel checks every index against -1 .. B-1 before it forms an address: nothing out of bounds is read"""
    be = backend()
    B = 7
    env, orc = make_pair(be, B, dict(rc.TINY, max_steps=30))
    eng = env.engines[0]
    env.reset(seed=6)
    orc.reset(seed=6)
    rng = np.random.default_rng(1)
    rc.play(env, orc, rng, 4)
    token, saved = env.snapshot(), rc.Saved(orc)
    rc.play(env, orc, rng, 4)
    index = np.array([3, B, 0, -2, 6, 2**31 - 1, 1], np.int32)
    assert eng.lib.rw_snapshot_restore_indexed(eng._h, token[0], C.c_void_p(be.ptr(index)), 0) == _capi.RW_OK
    with pytest.raises(_capi.EngineError, match="rw_snapshot_restore_indexed") as err:
        env.sync()
    assert err.value.code == _capi.RW_ERR_INVALID_ARG
    env.sync()                                               # the status word is clear again
    rc.rearrange(orc, saved, np.where((index < 0) | (index >= B), -1, index))
    lockstep.same_state(env.get_state(), orc.get_state(), "bad indices")
    env.free_snapshot(token)
    env.close()


# ------------------------------------------------------------------------------------------------ 6. GPU: the torch surface
@pytest.mark.gpu
def test_tensor_indices_of_restore_and_clone_envs():
    import torch

    B = 33
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1")
    env = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
    orc = OracleVecEnv(B, **kw)
    env.reset(seed=4)
    orc.reset(seed=4)
    rng = np.random.default_rng(2)
    rc.play(env, orc, rng, 6)
    token, saved = env.snapshot(), rc.Saved(orc)
    rc.play(env, orc, rng, 6)
    index = rc.index_pattern("random", B)
    idx32 = torch.from_numpy(index).cuda()
    obs = env.restore(token, index=idx32)
    assert obs.is_cuda and obs.data_ptr() == env.engines[0].device_array("obs").ptr
    rc.rearrange(orc, saved, index)
    env.sync()
    assert np.array_equal(obs.cpu().numpy(), orc.obs())
    lockstep.same_state(env.get_state(), orc.get_state(), "restore(tensor)")
    rc.play(env, orc, rng, 3)
    index = rc.index_pattern("reversal", B)
    saved = rc.Saved(orc)
    obs = env.clone_envs(torch.from_numpy(index.astype(np.int64)).cuda(), keep_rng=True)
    rc.rearrange(orc, saved, index, keep_rng=True)
    env.sync()
    assert np.array_equal(obs.cpu().numpy(), orc.obs())
    lockstep.same_state(env.get_state(), orc.get_state(), "clone_envs(int64 tensor)")
    before = orc.get_state()
    for bad in (idx32.cpu(), idx32[:-1], idx32.reshape(B, 1), idx32.float(), [idx32, idx32]) + \
            ((idx32.to("cuda:1"),) if torch.cuda.device_count() > 1 else ()):
        with pytest.raises(ValueError):
            env.restore(token, index=bad)
        with pytest.raises(ValueError):
            env.clone_envs(bad)
    env.sync()
    lockstep.same_state(env.get_state(), before, "a refused call has done nothing")
    env.free_snapshot(token)
    env.close()


@pytest.mark.gpu
def test_clone_envs_inside_a_captured_loop_reads_the_index_at_replay_time():
    """capture_loop(policy, steps=3): the policy clones by a device index tensor every round and plays a tape; the tensor is rewritten
    on the device between the two replays.  Capturing succeeds (a host synchronisation inside the capture would fail it); the replays
    equal an eager oracle loop that makes the same clones."""
    import torch

    B, N, K = 33, 4, 3
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1", max_steps=5)
    env = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
    orc = OracleVecEnv(B, **kw)
    env.reset(seed=7)
    orc.reset(seed=7)
    tape = np.random.default_rng(6).choice(5, size=(2 * K, B, N), p=rc.P_ACT).astype(np.int32)
    dev_tape = torch.from_numpy(tape).cuda()
    cursor = torch.zeros((), dtype=torch.long, device="cuda")
    indices = [rc.index_pattern("random", B), np.where(np.arange(B) % 2 == 0, (np.arange(B) * 7 + 3) % B, -1).astype(np.int32)]
    idx = torch.from_numpy(indices[0]).cuda()

    def policy(obs, rewards, terminated):
        env.clone_envs(idx, keep_rng=True)
        a = dev_tape.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return a

    loop = env.capture_loop(policy, steps=K, warmup=0)
    cursor.zero_()
    for r in range(2):
        idx.copy_(torch.from_numpy(indices[r]).cuda())
        loop.replay()
    torch.cuda.synchronize()
    ended = 0
    for r in range(2 * K):
        rc.rearrange(orc, rc.Saved(orc), indices[r // K], keep_rng=True)
        _, _, done = orc.step_autoreset(tape[r], "next_step")
        ended += int(done.sum())
    assert ended >= B
    v = env._torch_views()
    assert np.array_equal(v["obs"].cpu().numpy(), orc.obs())
    lockstep.same_state(env.get_state(), orc.get_state(), "two replays")
    env.close()
