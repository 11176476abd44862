"""Device-side seeding and masked reset: rw_seed_device / rw_reset_device, Engine.seed_device / reset_device, and the tensor paths of
WarehouseVecEnv.reset(seed=, mask=, options={"reset_mask": ...}), seed(seed, mask) and Pipeline.reset.

  - CPU suite: the product sources on host threads (tests/emu).  In that build a device pointer is a host pointer, so numpy arrays serve as
    the "device" arrays: the seed kernel against numpy itself, twin engines (rw_reset with host arrays beside rw_reset_device), lockstep
    against the oracle with "reset what just ended" after every step, RW_BUF_TERMINATED as the mask, the host layer's argument rules.
  - GPU suite (-m gpu): the same checks on the gfx950 library with torch tensors through the Python surface, a reset inside a captured
    loop (a host synchronisation inside the capture would fail it), and two pipelines.
Every comparison is exact (array_equal): seeding and reset are integer algorithms, pinned to numpy / the reference elsewhere."""
import ctypes as C

import numpy as np
import pytest

import lockstep
from device_backends import BACKENDS, GENERIC, Gpu, Host
from models import everything, same_everything
from rware_oracle import OracleVecEnv

import rware_amd
from rware_amd import _capi

M64 = (1 << 64) - 1
# 0, 1, the last one-word seed, the first with a high entropy word, another of those, the sign bit of an int64, all ones
SPECIAL = [0, 1, 2**32 - 1, 2**32, 2**32 + 5, 2**63, 2**64 - 1]
P_ACT = [.05, .7, .1, .1, .05]


def numpy_state(seed):
    st = np.random.PCG64(np.random.SeedSequence(int(seed))).state["state"]
    s, inc = st["state"], st["inc"]
    return np.array([s >> 64, s & M64, inc >> 64, inc & M64, 0, 0], dtype=np.uint64)


def make_env(be, env_id, B, **kw):
    return rware_amd.WarehouseVecEnv(B, library=be.library(), **dict(rware_amd.env_kwargs(env_id), **kw))


# ------------------------------------------------------------------------------------------------ 1. the seed kernel against numpy
def _mask_of(kind, B):
    return {"zeros": np.zeros(B, np.uint8), "ones": np.ones(B, np.uint8), "alternating": (np.arange(B) % 2).astype(np.uint8),
            "last": (np.arange(B) == B - 1).astype(np.uint8), "null": None}[kind]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["zeros", "ones", "alternating", "last", "null"])
@pytest.mark.parametrize("B", [7, 300])   # one partial block (a wrong stride of the [6][B] layout shows) / a second block
def test_seed_kernel_matches_numpy_and_leaves_masked_out_envs_alone(B, kind, backend):
    be = backend()
    env = make_env(be, "rware-tiny-2ag-v1", B)
    eng = env.engines[0]
    env.reset(seed=1)
    seeds = np.random.default_rng(B).integers(0, 2**63, size=B, dtype=np.uint64)
    # B = 300: special seeds on both sides of the wavefront and block boundaries and on the last env of the second block
    where = np.arange(7)[::-1].copy() if B == 7 else np.array([0, 41, 63, 64, 255, 256, B - 1])
    seeds[where] = np.array(SPECIAL, dtype=np.uint64)
    before = np.random.default_rng(5).integers(1, 2**63, size=(6, B), dtype=np.uint64)
    before[4] = 1                                    # has_uint32 set, a buffered half in uinteger
    before[5] = np.arange(B, dtype=np.uint64) + 77
    eng.write("rng", before)
    mask = _mask_of(kind, B)
    eng.seed_device(be.ptr(seeds), be.ptr(mask))
    got = eng.read("rng")
    assert got.shape == (6, B) and got.dtype == np.uint64
    for e in range(B):
        if mask is None or mask[e]:
            assert np.array_equal(got[:, e], numpy_state(seeds[e])), (e, hex(int(seeds[e])))
            assert got[4, e] == 0 and got[5, e] == 0
        else:
            assert np.array_equal(got[:, e], before[:, e]), e
    env.close()


# ------------------------------------------------------------------------------------------------ 2. twin engines: host path == device path
OPT_IN = dict(action_mask=True, episode_stats=True, stats=True)
TWINS = {
    "tiny-generic": ("rware-tiny-2ag-v1", 12, dict(GENERIC, **OPT_IN)),
    "small-exact": ("rware-small-4ag-v1", 32, {}),            # the ahead-of-time exact-shape build
    "small-opt-in": ("rware-small-4ag-v1", 32, dict(OPT_IN)),
    "image-uint8": ("rware-tiny-2ag-v1", 12, dict(GENERIC, observation_type=rware_amd.ObservationType.IMAGE, obs_format="uint8", **OPT_IN)),
    "packed": ("rware-tiny-2ag-v1", 12, dict(GENERIC, obs_format="packed", **OPT_IN)),
}


def warm_pair(be, env_id, B, kw, max_steps=6, mode="next_step", seed=3, steps=4):
    """two engines of one configuration in the same mid-episode state: staggered step counters, a few steps taken — some envs have just
    ended, the others have not; counters and episode statistics are non-zero"""
    pair = [make_env(be, env_id, B, max_steps=max_steps, autoreset_mode=mode, **kw) for _ in range(2)]
    N = pair[0].n_agents
    rng = np.random.default_rng(11)
    acts = rng.choice(5, size=(steps, B, N), p=P_ACT).astype(np.int32)
    for env in pair:
        env.reset(seed=seed)
        env.set_state(steps=(np.arange(B) % 4).astype(np.int32), refresh_obs=False)
        for a in acts:
            env.step(a)
    term = pair[0].engines[0].read("terminated")
    assert 0 < term.sum() < B, "the warm-up has to end some envs and not others"
    return pair, rng


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", ["seeds+mask", "mask", "seeds", "neither"])
@pytest.mark.parametrize("twin", list(TWINS))
def test_device_reset_equals_host_reset_on_a_twin_engine(twin, case, backend):
    be = backend()
    env_id, B, kw = TWINS[twin]
    (a, b), rng = warm_pair(be, env_id, B, kw)
    info = a.engines[0].info
    if twin == "small-exact":
        assert info.build_kind == 1 and info.jit == 0
    if "envs_per_workgroup" in kw:
        assert info.build_kind == 0 and info.envs_per_workgroup == 4 and info.n_workgroups == 3
    before = same_everything(a, b, "before the reset")
    if a.engines[0].episodes:
        assert before["ep_length"].any() and before["ep_count"].any()
    seeds = (np.uint64(2**32 - 3) + np.arange(B, dtype=np.uint64) * np.uint64(2**31)) if "seeds" in case else None
    mask = (np.arange(B) % 3 != 1).astype(np.uint8) if "mask" in case else None
    a.engines[0].reset(seeds, mask)                                  # rw_reset: host arrays
    b.engines[0].reset_device(be.ptr(seeds), be.ptr(mask))           # rw_reset_device: device arrays
    after = same_everything(a, b, case)
    hit = np.ones(B, bool) if mask is None else mask.astype(bool)
    assert not after["steps"][hit].any() and np.array_equal(after["steps"][~hit], before["steps"][~hit])
    if seeds is not None:   # the reseeded streams have drawn the reset already; the others kept their state bit for bit
        assert np.array_equal(after["rng"][~hit], before["rng"][~hit]) and not np.array_equal(after["rng"][hit], before["rng"][hit])
    for t in range(20):
        act = rng.choice(5, size=(B, a.n_agents), p=P_ACT).astype(np.int32)
        a.step(act)
        b.step(act)
        same_everything(a, b, (case, "step", t))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 3. lockstep against the oracle
class AsNumpy:
    """an output="torch" env seen through host arrays, for the lockstep harness"""

    def __init__(self, env):
        self.env = env

    def step(self, a):
        obs, rew, term, trunc, info = self.env.step(a)
        self.env.sync()
        return obs.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), {}

    def get_state(self):
        return self.env.get_state()


@pytest.mark.parametrize("backend", BACKENDS)
def test_reset_what_just_ended_through_the_device_path_in_lockstep_with_the_oracle(backend):
    """autoreset disabled, max_steps 6, episode ends staggered: after every step the ended envs are reset through the device path with
    mask = terminated and seeds 1000 k + e (emulated: rw_reset_device on host arrays; GPU: reset(seed=tensor, mask=<the zero-copy
    terminated tensor>)); 40 steps, every compared field exact"""
    be = backend()
    B, T = 10, 40
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1", max_steps=6)
    gpu = backend is Gpu
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), autoreset_mode="disabled", output="torch" if gpu else "numpy", **kw)
    orc = OracleVecEnv(B, **kw)
    env.reset(seed=21)
    orc.reset(seed=21)
    stagger = (np.arange(B) % 6).astype(np.int32)
    env.set_state(steps=stagger, refresh_obs=False)
    orc.set_state(steps=stagger)
    rng = np.random.default_rng(2)
    resets = []

    def on_step(t, obs, rew, term, info):
        term = np.asarray(term)
        if not term.any():
            return
        resets.append(int(term.sum()))
        if gpu:
            import torch

            flags = env.device_tensor("terminated").view(torch.bool)          # RW_BUF_TERMINATED itself
            seeds = torch.arange(1000 * t, 1000 * t + B, dtype=torch.int64, device="cuda")
            o = env.reset(seed=seeds, mask=flags)[0].cpu().numpy()
        else:
            seeds = np.uint64(1000 * t) + np.arange(B, dtype=np.uint64)
            env.engines[0].reset_device(be.ptr(seeds), be.ptr(term.astype(np.uint8)))
            o = env.observations()
        lockstep.same_obs(o, orc.reset(seed=1000 * t, mask=term.astype(np.uint8)), "masked reset obs", t)
        lockstep.same_state(env.get_state(), orc.get_state(), t)

    run = lockstep.lockstep(AsNumpy(env) if gpu else env, orc, lambda t: rng.choice(5, size=(B, 2), p=P_ACT).astype(np.int32), "disabled",
                            seed=None, steps=T, state_every=1, on_step=on_step)
    assert run.steps == T and len(resets) >= 20 and sum(resets) >= 4 * B
    env.close()


# ------------------------------------------------------------------------------------------------ 4. the mask may be RW_BUF_TERMINATED
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("twin", ["tiny-generic", "small-exact"])
def test_the_terminated_buffer_itself_can_be_the_mask(twin, backend):
    be = backend()
    env_id, B, kw = TWINS[twin]
    (a, b), _ = warm_pair(be, env_id, B, kw, mode="disabled")
    before = same_everything(a, b, "before the reset")
    flags = before["buf:terminated"].copy()
    seeds = np.uint64(5000) + np.arange(B, dtype=np.uint64)
    a.engines[0].reset_device(be.ptr(seeds), be.ptr(flags))                                          # a copy of the flags
    b.engines[0].reset_device(be.ptr(seeds), b.engines[0].device_array("terminated").ptr)            # the buffer the launch rewrites
    after = same_everything(a, b, "aliased mask")
    hit = flags.astype(bool)
    assert not after["steps"][hit].any() and np.array_equal(after["steps"][~hit], before["steps"][~hit])
    for k in ("grid", "agent_x", "agent_y", "agent_dir", "queue", "rng"):
        assert np.array_equal(after[k][~hit], before[k][~hit]), k
    want = OracleVecEnv(B, **lockstep.oracle_kwargs(env_id))       # the reseeded envs: what reset(seed=5000 + e) gives
    want.reset(seed=5000)
    for k in ("grid", "agent_x", "agent_y", "agent_dir", "queue", "rng"):
        assert np.array_equal(after[k][hit], want.get_state()[k][hit]), k
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5. the host layer
def test_options_reset_mask_is_the_mask_argument():
    B = 9
    envs = [make_env(Host, "rware-tiny-2ag-v1", B, max_steps=5, **GENERIC) for _ in range(2)]
    m = (np.arange(B) % 2).astype(bool)
    for env in envs:
        env.reset(seed=4)
        env.step(np.ones((B, 2), np.int32))
    oa, _ = envs[0].reset(seed=90, mask=m)
    ob, _ = envs[1].reset(seed=90, options={"reset_mask": m, "something_else": 1})
    assert np.array_equal(oa, ob)
    st = same_everything(envs[0], envs[1], "options")
    assert np.array_equal(st["steps"] == 0, m)
    with pytest.raises(ValueError):
        envs[0].reset(mask=m, options={"reset_mask": m})
    envs[0].reset(options={})                      # other / no keys: a plain reset of every env
    envs[0].reset(options={"reset_mask": None})
    assert not envs[0].get_state()["steps"].any()
    for env in envs:
        env.close()


def test_a_reset_without_tensors_goes_through_rw_reset_as_before():
    env = make_env(Host, "rware-tiny-2ag-v1", 5, **GENERIC)
    eng, calls = env.engines[0], []
    plain = eng.reset
    eng.reset = lambda *a: (calls.append(a), plain(*a))[1]
    eng.reset_device = eng.seed_device = lambda *a: pytest.fail("the device path was taken without a tensor")
    env.reset(seed=3)
    env.reset()
    env.reset(seed=[5, 6, 7, 8, 9], mask=[1, 0, 1, 0, 1])
    env.reset(options={"reset_mask": np.array([0, 1, 0, 0, 0], bool)})
    env.seed(12)
    assert len(calls) == 4 and calls[1] == (None, None) and calls[3][0] is None and calls[3][1].tolist() == [0, 1, 0, 0, 0]
    assert np.array_equal(env.get_state()["rng"][2], numpy_state(14))
    env.close()


def test_entry_points_check_their_arguments():
    env = make_env(Host, "rware-tiny-2ag-v1", 6, **GENERIC)
    eng = env.engines[0]
    env.reset(seed=1)
    before = eng.read("rng")
    seeds = np.arange(8, dtype=np.uint64)
    assert seeds.ctypes.data % 8 == 0
    inv = _capi.RW_ERR_INVALID_ARG
    odd = C.c_void_p(seeds.ctypes.data + 4)
    assert eng.lib.rw_reset_device(eng._h, odd, None) == inv and eng.lib.rw_seed_device(eng._h, odd, None) == inv
    assert eng.lib.rw_seed_device(eng._h, None, None) == inv
    assert eng.lib.rw_reset_device(None, None, None) == inv and eng.lib.rw_seed_device(None, C.c_void_p(seeds.ctypes.data), None) == inv
    with pytest.raises(_capi.EngineError):
        eng.seed_device(seeds.ctypes.data + 1)
    assert np.array_equal(eng.read("rng"), before)   # a refused call has done nothing
    assert eng.lib.rw_reset_device(eng._h, None, None) == _capi.RW_OK
    env.close()


def test_tensors_are_refused_where_nothing_orders_them():
    """a host (CPU) tensor is a tensor on another device; an output="numpy" env enqueues on a stream of its own: ValueError, nothing reset"""
    torch = pytest.importorskip("torch")
    env = make_env(Host, "rware-tiny-2ag-v1", 4, **GENERIC)
    env.reset(seed=1)
    env.step(np.ones((4, 2), np.int32))
    for kw in (dict(seed=torch.arange(4)), dict(mask=torch.ones(4, dtype=torch.bool)), dict(options={"reset_mask": torch.ones(4, dtype=torch.uint8)}),
               dict(seed=[torch.arange(4)])):
        with pytest.raises(ValueError):
            env.reset(**kw)
    with pytest.raises(ValueError):
        env.seed(torch.arange(4))
    with pytest.raises(ValueError):
        env.seed(3, mask=np.ones(4, bool))
    assert env.get_state()["steps"].tolist() == [1, 1, 1, 1]
    env.close()


@pytest.mark.gpu
def test_tensor_arguments_of_reset_and_seed():
    import torch

    B = 12
    kw = dict(rware_amd.env_kwargs("rware-tiny-2ag-v1"), max_steps=5)
    dev = [rware_amd.WarehouseVecEnv(B, output="torch", **kw) for _ in range(3)]
    ref = rware_amd.WarehouseVecEnv(B, **kw)
    base = 2**40 + 17
    vals = base + np.arange(B, dtype=np.int64)
    m = (np.arange(B) % 3 == 0)
    for env in dev + [ref]:
        env.reset(seed=1)
        env.step(np.ones((B, 2), np.int32))
    want_obs, _ = ref.reset(seed=base, mask=m)
    mask_t = torch.from_numpy(m).cuda()
    # an int64 tensor of non-negative seeds == the same values as uint64 == a Python int beside a device mask (env i: seed + i)
    o0, info = dev[0].reset(seed=torch.from_numpy(vals).cuda(), mask=mask_t)
    assert info == {} and o0.is_cuda and o0.data_ptr() == dev[0].engines[0].device_array("obs").ptr
    o1, _ = dev[1].reset(seed=torch.from_numpy(vals.astype(np.uint64).view(np.int64)).cuda().view(torch.uint64), mask=mask_t.to(torch.uint8))
    o2, _ = dev[2].reset(seed=base, options={"reset_mask": mask_t})
    want = ref.get_state()
    for env, o in zip(dev, (o0, o1, o2)):
        env.sync()
        assert np.array_equal(o.cpu().numpy(), want_obs)
        lockstep.same_state(env.get_state(), want)
    # a host sequence beside a device mask is uploaded; a host mask beside device seeds too
    want_obs, _ = ref.reset(seed=vals[::-1].copy(), mask=~m)
    o0, _ = dev[0].reset(seed=vals[::-1].copy(), mask=(~mask_t))
    o1, _ = dev[1].reset(seed=torch.from_numpy(vals[::-1].copy()).cuda(), mask=~m)
    for env, o in zip(dev[:2], (o0, o1)):
        env.sync()
        assert np.array_equal(o.cpu().numpy(), want_obs)
        lockstep.same_state(env.get_state(), ref.get_state())
    # int64 -1 is reinterpreted: 2**64 - 1
    dev[0].seed(torch.full((B,), -1, dtype=torch.int64, device="cuda"))
    dev[0].sync()
    assert all(np.array_equal(row, numpy_state(M64)) for row in dev[0].get_state()["rng"])
    # seed(tensor) == seed(int) for int + arange; seed(int, mask=tensor) reseeds the masked envs only
    ref.seed(777)
    dev[0].seed(torch.arange(777, 777 + B, device="cuda"))
    keep = dev[1].get_state()["rng"]
    dev[1].seed(777, mask=mask_t)
    dev[0].sync(); dev[1].sync()
    assert np.array_equal(dev[0].get_state()["rng"], ref.get_state()["rng"])
    got = dev[1].get_state()["rng"]
    assert np.array_equal(got[m], ref.get_state()["rng"][m]) and np.array_equal(got[~m], keep[~m])
    # what is refused, before anything is enqueued
    good = torch.arange(B, device="cuda")
    for bad in (dict(seed=good[:-1]), dict(seed=good.reshape(B, 1)), dict(seed=good.to(torch.int32)), dict(seed=good.float()),
                dict(mask=torch.ones(B, dtype=torch.int32, device="cuda")), dict(mask=torch.ones(B + 1, dtype=torch.bool, device="cuda")),
                dict(seed=good.cpu()), dict(seed=good, mask=torch.ones(B, dtype=torch.bool)), dict(seed=[good, good]),
                dict(seed=2**63 - B + 1, mask=mask_t), dict(seed=-1, mask=mask_t), dict(mask=mask_t, options={"reset_mask": mask_t})):
        with pytest.raises(ValueError):
            dev[2].reset(**bad)
    dev[2].reset(seed=2**63 - B, mask=mask_t)   # the largest base an int64 arange holds
    dev[2].sync()
    assert np.array_equal(dev[2].get_state()["rng"][0], _reset_rng(2**63 - B, kw))
    for env in dev + [ref]:
        env.close()


def _reset_rng(seed, kw):
    o = OracleVecEnv(1, **lockstep.oracle_kwargs(None, **kw))
    o.reset(seed=seed)
    return o.get_state()["rng"][0]


# ------------------------------------------------------------------------------------------------ 6. GPU: a reset inside a captured loop
@pytest.mark.gpu
def test_a_reset_with_device_seeds_and_mask_is_captured_with_the_loop():
    """capture_loop(policy, steps=4): the policy restarts what just ended — reset(seed=counter + arange, mask=terminated), both on the
    device — and plays a tape.  Capturing succeeds (a host synchronisation inside the capture would fail it); three replays equal an
    eager oracle loop that does the same resets."""
    import torch

    B, N, K, R = 32, 4, 4, 3
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1", max_steps=3)
    env = rware_amd.WarehouseVecEnv(B, output="torch", autoreset_mode="disabled", **kw)
    orc = OracleVecEnv(B, **kw)
    env.reset(seed=7)
    orc.reset(seed=7)
    stagger = (np.arange(B) % 3).astype(np.int32)
    env.set_state(steps=stagger, refresh_obs=False)
    orc.set_state(steps=stagger)
    tape = np.random.default_rng(6).choice(5, size=(K * R, B, N), p=P_ACT).astype(np.int32)
    dev_tape = torch.from_numpy(tape).cuda()
    cursor = torch.zeros((), dtype=torch.long, device="cuda")
    counter = torch.zeros((), dtype=torch.int64, device="cuda")
    ar = torch.arange(B, dtype=torch.int64, device="cuda")
    rounds = torch.zeros((K * R, B), dtype=torch.uint8, device="cuda")     # the mask every round's reset saw

    def policy(obs, rewards, terminated):
        rounds.index_copy_(0, cursor.reshape(1), terminated.view(torch.uint8).unsqueeze(0))
        env.reset(seed=counter + ar, mask=terminated)
        counter.add_(1000)
        a = dev_tape.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return a

    loop = env.capture_loop(policy, steps=K, warmup=0)
    cursor.zero_(); counter.zero_(); rounds.zero_()
    for _ in range(R):
        loop.replay()
    torch.cuda.synchronize()
    done, ended = np.zeros(B, np.uint8), 0
    seen = rounds.cpu().numpy()
    for r in range(K * R):
        assert np.array_equal(seen[r], done), r
        if done.any():
            orc.reset(seed=1000 * r, mask=done)
        o, rew, done = orc.step_autoreset(tape[r], "disabled")
        ended += int(done.sum())
    assert ended >= 3 * B
    v = env._torch_views()
    assert np.array_equal(v["obs"].cpu().numpy(), o) and np.array_equal(v["rewards"].cpu().numpy(), rew)
    assert np.array_equal(v["terminated"].cpu().numpy(), done)
    lockstep.same_state(env.get_state(), orc.get_state())
    env.close()


# ------------------------------------------------------------------------------------------------ 7. GPU: pipelines
@pytest.mark.gpu
def test_pipelines_reset_with_device_tensors_equal_the_whole_batch():
    import torch

    B = 64
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
    pipes = rware_amd.make_pipelines(B, 2, **kw)
    whole = rware_amd.WarehouseVecEnv(B, **kw)
    seeds = np.random.default_rng(8).integers(0, 2**63, size=B, dtype=np.int64)
    m = np.arange(B) % 4 != 2
    for p in pipes:
        p.reset(seed=5)
    whole.reset(seed=5)
    want_obs, _ = whole.reset(seed=seeds.astype(np.uint64), mask=m)
    st = whole.get_state()
    seeds_t, mask_t = torch.from_numpy(seeds).cuda(), torch.from_numpy(m).cuda()
    torch.cuda.synchronize()
    for p in pipes:
        obs, _ = p.reset(seed=seeds_t[p.lo:p.hi], mask=mask_t[p.lo:p.hi])
        p.stream.synchronize()
        assert np.array_equal(obs.cpu().numpy(), want_obs[p.lo:p.hi])
        got = p.env.get_state()
        for k in got:
            assert np.array_equal(got[k], st[k][p.lo:p.hi]), k
    for p in pipes:
        p.env.close()
    whole.close()
