"""rw_global_image: Warehouse.get_global_image built on the device — the kernel, Engine.global_image and
WarehouseVecEnv.global_image_device.

  - CPU suite: the product sources on host threads (tests/emu; a device pointer is a host pointer there, so numpy arrays serve as the
    "device" arrays), the generic step kernel on 4-env workgroups.
  - GPU suite (-m gpu): the same checks on the gfx950 library with torch tensors as the device arrays, then the torch surface: the
    cached result tensor, `out=`, a call inside a captured loop (a host synchronisation inside the capture would fail it).
Expectations: the UNMODIFIED reference's own images (tests/golden/global_image, written by tests/golden/generate_global_image.py), and
the host form global_image_from_state, which tests/test_oracle_vs_reference.py pins to the reference.  Every comparison is exact
(array_equal): an image is integers 0 .. 4."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_util as gu
import lockstep
from device_backends import BACKENDS, GENERIC, GUARD, POISON, emu_library
from models import ALL7, PLAIN
from rware_oracle import OracleVecEnv

import rware_amd
from rware_amd import _capi
from rware_amd.vector_env import global_image_from_state

P_ACT = [.05, .7, .1, .1, .05]
F32, U8 = np.dtype(np.float32), np.dtype(np.uint8)


def device_image(be, eng, layers, pad=None, dtype=F32, shift=0):
    """rw_global_image into a poisoned device array that starts `shift` bytes behind a 16-byte boundary -> (image, raised): the image
    (B, C', H', W'); whether the following sync() raised IndexError.  The bytes in front of and behind the image must be untouched."""
    dtype = np.dtype(dtype)
    shape = (eng.B,) + (tuple(pad) if pad is not None else (len(layers), eng.H, eng.W))
    nbytes = int(np.prod(shape)) * dtype.itemsize
    keep, base, read = be.alloc(GUARD + shift + nbytes + GUARD)
    eng.global_image(layers, base + GUARD + shift, pad, dtype)
    _, raised = lockstep.attempt(eng.sync)
    eng.sync()                                       # the status word is clear again
    raw = read()
    lo = GUARD + shift
    assert (raw[:lo] == POISON).all() and (raw[lo + nbytes:] == POISON).all(), "bytes outside the image were written"
    return raw[lo:lo + nbytes].view(dtype).reshape(shape).copy(), raised


def lenient_plane(st, layer):
    """AGENT_DIRECTION / AGENT_LOAD as the reference writes them (`layer[ag.x, ag.y]`, the last agent winning), except that an agent
    outside the transposed bounds writes nothing — what the kernel leaves where the reference raises"""
    B, _, H, W = st["grid"].shape
    out = np.zeros((B, H, W), np.float32)
    for b in range(B):
        for i in range(st["agent_x"].shape[1]):
            x, y = int(st["agent_x"][b, i]), int(st["agent_y"][b, i])
            if (layer == 4 and st["agent_carry"][b, i] <= 0) or x >= H or y >= W:
                continue
            out[b, x, y] = st["agent_dir"][b, i] + 1 if layer == 3 else 1
    return out


def want_image(st, goals, layers, pad=None):
    """(image, raised): the host form; where it raises, the transposed planes without the agents that made it raise"""
    whole, raised = lockstep.attempt(lambda: global_image_from_state(st, goals, layers, pad))
    if not raised:
        return whole, False
    planes = [lenient_plane(st, l) if l in (3, 4) else global_image_from_state(st, goals, [l])[:, 0] for l in layers]
    img = np.stack(planes, axis=1)
    if pad is not None:
        d = [p - s for p, s in zip(pad, img.shape[1:])]
        img = np.pad(img, ((0, 0),) + tuple((k // 2, k - k // 2) for k in d))
    return img, True


def check(be, env, st, layers, pad=None, dtype=F32, shift=0, what=None):
    got, raised = device_image(be, env.engines[0], layers, pad, dtype, shift)
    want, want_raised = want_image(st, env.goals, layers, pad)
    assert got.dtype == dtype and got.shape == want.shape, (what, got.shape, want.shape)
    assert raised == want_raised, (what, layers, "IndexError", raised, want_raised)
    assert np.array_equal(got, want.astype(dtype)), (what, layers, pad, dtype, shift, np.argwhere(got != want)[:5].tolist())
    return raised


# ------------------------------------------------------------------------------------------------ 1. the reference's own images
FIXTURE = os.path.join(gu.GOLDEN_DIR, "global_image", "global_image.npz")
REPLAYS = {"img-square-all7-msg1": [ALL7], "layoutstr-3ag": [ALL7], "tiny-2ag": [PLAIN, [3], [4]]}


@pytest.fixture(scope="module")
def golden_images():
    z = np.load(FIXTURE, allow_pickle=False)
    return {k: z[k] for k in z.files if k != "meta"}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(REPLAYS))
def test_every_step_of_a_golden_trace_gives_the_image_of_the_reference(name, backend, golden_images):
    be = backend()
    meta, z = gu.load_fixture(name)
    env = rware_amd.WarehouseVecEnv(meta["E"], library=be.library(), **dict(gu.ctor_kwargs(meta), **be.kw))
    eng = env.engines[0]
    if not be.gpu:
        assert eng.info.build_kind == 0 and eng.info.envs_per_workgroup == 4
    env.reset(seed=meta["seed"])
    steps = {tuple(ls): [0, 0] for ls in REPLAYS[name]}             # per layer list: steps without / with an IndexError
    for t in range(meta["T"]):
        _, rew, done, _, _ = env.step(z["actions"][t].astype(np.int32))
        assert np.array_equal(rew, z["rewards"][t]) and np.array_equal(done.astype(np.uint8), z["done"][t]), t
        for ls in REPLAYS[name]:
            key = name + "/" + "-".join(map(str, ls))
            want, want_raised = golden_images[key + "/image"][t], bool(golden_images[key + "/raised"][t].any())
            for dtype in (F32, U8):
                got, raised = device_image(be, eng, ls, dtype=dtype)
                assert raised == want_raised, (key, t, dtype)
                if not raised:
                    assert np.array_equal(got, want.astype(dtype)), (key, t, dtype, np.argwhere(got != want)[:5].tolist())
            steps[tuple(ls)][want_raised] += 1
    for ls, (clean, raising) in steps.items():
        assert clean + raising == meta["T"]
        if name == "tiny-2ag" and ls in ((3,), (4,)):
            assert clean > 100 and raising > 100, "the fixture has to hold both kinds of step"
        else:
            assert raising == 0
    env.close()


# ------------------------------------------------------------------------------------------------ 2. lockstep against the oracle
# tiny is 11 x 10 = 110 cells: a one-layer float image is 110 floats per env, so 16-byte stores straddle env boundaries
SHAPES = {
    "tiny-7": (7, dict(shelf_columns=3, column_height=8, shelf_rows=1, n_agents=2), [PLAIN, [1], [3], [4], ALL7]),   # one ragged workgroup
    "tiny-300": (300, dict(shelf_columns=3, column_height=8, shelf_rows=1, n_agents=2), [PLAIN, [3]]),               # several workgroups, the last ragged
    "wide-4x16": (9, dict(shelf_columns=5, column_height=1, shelf_rows=1, n_agents=3), [PLAIN, [3], [4, 2], ALL7]),  # W > H: the x >= H side
    "29x28-10ag": (5, dict(shelf_columns=9, column_height=8, shelf_rows=3, n_agents=10), [PLAIN, ALL7, [4], [1, 3]]),  # > 255 shelves: uint16 shadow
}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forty_steps_with_a_masked_reset_in_lockstep_with_the_oracle(shape, backend):
    be = backend()
    B, kw, lists = SHAPES[shape]
    kw = lockstep.oracle_kwargs(None, max_steps=30, **kw)
    geom = dict(be.kw, envs_per_workgroup=32) if be.kw and B == 300 else be.kw    # (emulated: a thread per lane — fewer, larger workgroups)
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), **dict(kw, **geom))
    orc = OracleVecEnv(B, **kw)
    eng = env.engines[0]
    assert (eng.H, eng.W) == {"tiny-7": (11, 10), "tiny-300": (11, 10), "wide-4x16": (4, 16), "29x28-10ag": (29, 28)}[shape]
    assert (eng.S > 255) == (shape == "29x28-10ag")
    lockstep.same_obs(env.reset(seed=5)[0], orc.reset(seed=5), "reset obs")
    rng = np.random.default_rng(3)
    seen = {False: 0, True: 0}
    for t in range(40):
        if t == 20:      # a masked reset in the middle: the image follows the reset envs
            m = (np.arange(B) % 3 == 0).astype(np.uint8)
            lockstep.same_obs(env.reset(seed=900, mask=m)[0], orc.reset(seed=900, mask=m), "masked reset obs", t)
        else:
            a = rng.choice(5, size=(B, env.n_agents), p=P_ACT).astype(np.int32)
            obs, rew, term, _, _ = env.step(a)
            o2, r2, d2 = orc.step_autoreset(a, "next_step")
            lockstep.same_obs(obs, o2, "obs", t)
        st = orc.get_state()
        for k, ls in enumerate(lists):
            seen[check(be, env, st, ls, dtype=(F32, U8)[(t + k) % 2], what=(shape, t))] += 1
    assert seen[False] >= 40
    if shape != "29x28-10ag":    # (29 x 28: an agent reaches y >= 28 only in the bottom row)
        assert seen[True] > 0, "no state of this run left the transposed bounds"
    lockstep.same_state(env.get_state(), orc.get_state(), 40)
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_sharded_env_gathers_the_images_of_its_engines(backend):
    be = backend()
    B = 10
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1")
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), devices=[0, 0, 0], **dict(kw, **be.kw))
    orc = OracleVecEnv(B, **kw)
    assert [e.B for e in env.engines] == [4, 3, 3]
    env.reset(seed=8)
    orc.reset(seed=8)
    rng = np.random.default_rng(4)
    seen = {False: 0, True: 0}
    for t in range(40):
        a = rng.choice(5, size=(B, 2), p=P_ACT).astype(np.int32)
        env.step(a)
        orc.step_autoreset(a, "next_step")
        st = orc.get_state()
        for ls, dtype, pad in ((PLAIN, "float32", None), ([3, 0], "uint8", (3, 12, 13)), ([4, 2], "uint8", None)):
            got, raised = lockstep.attempt(lambda: env.global_image_device(ls, pad_to_shape=pad, dtype=dtype))
            want, want_raised = lockstep.attempt(lambda: global_image_from_state(st, env.goals, ls, pad))
            assert raised == want_raised, (t, ls)
            seen[raised] += 1
            if not raised:
                assert got.dtype == np.dtype(dtype) and got.shape == want.shape and np.array_equal(got, want), (t, ls)
    assert seen[True] > 0 and seen[False] > 40, seen
    env.sync()           # the IndexError was consumed where it was raised
    env.close()


# ------------------------------------------------------------------------------------------------ 3. padding and addressing
@pytest.fixture(params=BACKENDS)
def played(request):
    """a tiny-2ag batch of 5 a few steps into its episodes, its backend and its state"""
    be = request.param()
    env = rware_amd.WarehouseVecEnv(5, library=be.library(), **dict(rware_amd.env_kwargs("rware-tiny-2ag-v1"), **be.kw))
    env.reset(seed=12)
    rng = np.random.default_rng(9)
    for _ in range(6):
        env.step(rng.choice(5, size=(5, 2), p=P_ACT).astype(np.int32))
    yield be, env, env.get_state()
    env.close()


def test_padding_is_split_like_the_reference_on_all_three_axes(played):
    be, env, st = played
    for layers, pad in ((PLAIN, (5, 11, 10)), (PLAIN, (6, 14, 12)), (PLAIN, (7, 13, 15)), ([0, 6], (8, 12, 11)), ([2], (1, 11, 17)), ([5, 1, 0], (4, 11, 10))):
        for dtype in (F32, U8):
            assert not check(be, env, st, layers, pad, dtype, what="pad")


def test_an_output_off_the_sixteen_byte_boundary_is_written_exactly(played):
    """every element of `out` and nothing else: the poison in front of and behind the image survives (device_image asserts it)"""
    be, env, st = played
    for dtype, shifts in ((F32, (4, 8, 12)), (U8, (1, 2, 7, 15))):
        for shift in shifts:
            for layers, pad in ((PLAIN, None), ([1], None), ([0, 2], (3, 12, 11))):
                assert not check(be, env, st, layers, pad, dtype, shift, what="shift")


def test_duplicated_layers_and_eight_layers(played):
    be, env, st = played
    for layers in ([0, 0, 6], [6, 6], [0, 1, 2, 5, 6, 0, 1, 2], [5] * 8):
        for dtype in (F32, U8):
            assert not check(be, env, st, layers, None, dtype, what="dup")


# ------------------------------------------------------------------------------------------------ 4. injected state
@pytest.mark.parametrize("backend", BACKENDS)
def test_two_agents_on_one_cell_and_a_carried_requested_shelf(backend):
    be = backend()
    B = 3
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), n_agents=3, **dict(
        {k: v for k, v in rware_amd.env_kwargs("rware-tiny-2ag-v1").items() if k != "n_agents"}, **be.kw))
    env.reset(seed=2)
    st = env.get_state()
    ys, xs = np.nonzero(st["grid"][0, 1])
    y, x = int(ys[0]), int(xs[0])                          # a cell with a shelf, inside the transposed bounds
    assert x < env.grid_size[0] and y < env.grid_size[1]
    shelf = st["grid"][:, 1, y, x].copy()
    ax, ay, ad, ac, q = (st[k].copy() for k in ("agent_x", "agent_y", "agent_dir", "agent_carry", "queue"))
    ax[:, :2], ay[:, :2] = x, y                            # agents 0 and 1 share the cell; agent 2 stands in the corner
    ax[:, 2], ay[:, 2] = 0, 0
    ad[:, 0], ad[:, 1], ad[:, 2] = 3, 1, 0
    ac[:] = 0
    ac[0, 1], ac[1, 0] = shelf[0], shelf[1]                # env 0: the higher index carries, env 1: the lower one, env 2: nobody
    q[:, 0] = shelf                                        # ... and the carried shelf is a requested one
    q[:, 1] = np.where(q[:, 1] == shelf, shelf % env.n_shelves + 1, q[:, 1])
    env.set_state(agent_x=ax, agent_y=ay, agent_dir=ad, agent_carry=ac, queue=q)
    st = env.get_state()
    for dtype in (F32, U8):
        got, raised = device_image(be, env.engines[0], ALL7, dtype=dtype)
        assert not raised
        assert np.array_equal(got, global_image_from_state(st, env.goals, ALL7).astype(dtype))
        assert (got[:, 3, x, y] == 2).all(), "AGENT_DIRECTION: the highest agent index wins the shared (mirrored) cell"
        assert got[:, 4, x, y].tolist() == [1, 1, 0] and (got[:, 1, y, x] == 1).all() and (got[:, 0, y, x] == 1).all()
    env.close()


# ------------------------------------------------------------------------------------------------ 5. arguments
def test_the_entry_point_checks_its_arguments():
    env = rware_amd.WarehouseVecEnv(6, library=emu_library(), **dict(rware_amd.env_kwargs("rware-tiny-2ag-v1"), **GENERIC))
    eng = env.engines[0]
    env.reset(seed=1)
    out = np.full(6 * 8 * 16 * 16 + 16, 7.0, np.float32)
    ptr = C.c_void_p(out.ctypes.data)
    i32x = lambda *v: (C.c_int32 * len(v))(*v)
    call = eng.lib.rw_global_image
    inv = _capi.RW_ERR_INVALID_ARG
    good = i32x(0, 5)
    assert call(None, good, 2, None, 0, ptr) == inv
    assert call(eng._h, None, 2, None, 0, ptr) == inv and call(eng._h, good, 2, None, 0, None) == inv
    assert call(eng._h, good, 0, None, 0, ptr) == inv and call(eng._h, i32x(*[0] * 9), 9, None, 0, ptr) == inv
    assert call(eng._h, i32x(0, 7), 2, None, 0, ptr) == inv and call(eng._h, i32x(-1), 1, None, 0, ptr) == inv
    for pad in ((1, 11, 10), (2, 10, 10), (2, 11, 9)):
        assert call(eng._h, good, 2, i32x(*pad), 0, ptr) == inv
    assert call(eng._h, good, 2, None, 2, ptr) == inv and call(eng._h, good, 2, None, -1, ptr) == inv
    assert call(eng._h, good, 2, None, 0, C.c_void_p(out.ctypes.data + 2)) == inv          # a float array at an odd address
    assert call(eng._h, good, 2, i32x(8, 65536, 65536), 1, ptr) == inv                     # 2^35 elements per env
    assert "slice it" in eng.lib.rw_last_error(eng._h).decode()
    assert (out == 7.0).all()                                                               # a refused call has done nothing
    eng.sync()
    assert call(eng._h, good, 2, i32x(2, 11, 10), 0, ptr) == _capi.RW_OK
    with pytest.raises(_capi.EngineError):
        eng.global_image([0, 9], out.ctypes.data)
    with pytest.raises(ValueError):
        eng.global_image([0], out.ctypes.data, dtype=np.float64)
    # the Python surface: the reference's AssertionError (:1028) and ValueError (:1018)
    for pad in ((1, 11, 10), (2, 10, 10), (2, 11, 9)):
        with pytest.raises(AssertionError):
            env.global_image_device(pad_to_shape=pad)
    with pytest.raises(ValueError):
        env.global_image_device([0, 7])
    with pytest.raises(ValueError):
        env.global_image_device(dtype="float64")
    with pytest.raises(ValueError):
        env.global_image_device(out=out)                  # `out` is a device tensor of output="torch" envs
    img = env.global_image_device()                       # the reference's default layers: SHELVES, GOALS
    assert img.dtype == np.float32 and np.array_equal(img, env.get_global_image(recompute=True))
    env.close()


def test_get_global_image_keeps_its_cache_beside_the_device_form():
    env = rware_amd.WarehouseVecEnv(4, library=emu_library(), **dict(rware_amd.env_kwargs("rware-tiny-2ag-v1"), **GENERIC))
    env.reset(seed=3)
    first = env.get_global_image(PLAIN)
    env.step(np.ones((4, 2), np.int32))
    dev = env.global_image_device(PLAIN, dtype="uint8")
    assert env.get_global_image(PLAIN) is first and env.global_image is first          # the cache: still the pre-step image
    fresh = env.get_global_image(PLAIN, recompute=True)
    assert fresh.dtype == np.float32 and not np.array_equal(fresh, first) and np.array_equal(dev, fresh.astype(np.uint8))
    env.close()


# ------------------------------------------------------------------------------------------------ 6. GPU: the torch surface
@pytest.mark.gpu
def test_torch_output_is_a_cached_cuda_tensor_equal_to_the_host_form():
    import torch

    B = 33
    env = rware_amd.WarehouseVecEnv(B, output="torch", **rware_amd.env_kwargs("rware-small-4ag-v1"))
    env.reset(seed=4)
    rng = np.random.default_rng(1)
    for t in range(12):
        env.step(rng.choice(5, size=(B, 4), p=P_ACT).astype(np.int32))
        img = env.global_image_device(PLAIN)
        u8 = env.global_image_device(PLAIN, dtype="uint8", pad_to_shape=(6, 21, 12))
        assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (B, 5, 20, 10) and u8.dtype == torch.uint8
        assert env.global_image_device(PLAIN) is img                      # allocated once per (layers, shape, dtype)
        env.sync()
        want = env.get_global_image(PLAIN, recompute=True)
        assert isinstance(want, np.ndarray) and env.global_image is want   # the host form and its cache are what they were
        assert np.array_equal(img.cpu().numpy(), want)
        assert np.array_equal(u8.cpu().numpy(), env.get_global_image(PLAIN, recompute=True, pad_to_shape=(6, 21, 12)).astype(np.uint8))
    big = torch.zeros(B * 5 * 200 + 8, device="cuda")
    out = big[1:1 + B * 5 * 200].view(B, 5, 20, 10)                        # 4 bytes behind a 16-byte boundary
    assert env.global_image_device(PLAIN, out=out) is out
    env.sync()
    assert np.array_equal(out.cpu().numpy(), want) and big[0] == 0 and (big[1 + B * 5 * 200:] == 0).all()
    for bad in (out[:-1], out.to(torch.uint8), out.cpu(), out.transpose(2, 3)):
        with pytest.raises(ValueError):
            env.global_image_device(PLAIN, out=bad)
    env.global_image_device([3])          # small is 20 x 10: after a few steps somebody stands at y >= 10
    with pytest.raises(IndexError):
        env.sync()
    env.close()


@pytest.mark.gpu
def test_a_call_inside_a_captured_loop_is_replayed_with_it():
    import torch

    B, N, K = 32, 4, 3
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1")
    env = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
    orc = OracleVecEnv(B, **kw)
    env.reset(seed=7)
    orc.reset(seed=7)
    tape = np.random.default_rng(6).choice(5, size=(2 * K, B, N), p=P_ACT).astype(np.int32)
    dev_tape = torch.from_numpy(tape).cuda()
    cursor = torch.zeros((), dtype=torch.long, device="cuda")
    img = torch.zeros((B, 5, 20, 10), dtype=torch.uint8, device="cuda")     # the preallocated `out`
    hist = torch.zeros((2 * K,) + tuple(img.shape), dtype=torch.uint8, device="cuda")

    def policy(obs, rewards, terminated):
        env.global_image_device(PLAIN, dtype="uint8", out=img)               # the state this round's observation describes
        hist.index_copy_(0, cursor.reshape(1), img.unsqueeze(0))
        a = dev_tape.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return a

    loop = env.capture_loop(policy, steps=K, warmup=0)
    cursor.zero_()
    hist.zero_()
    for _ in range(2):
        loop.replay()
    torch.cuda.synchronize()
    seen = hist.cpu().numpy()
    for r in range(2 * K):
        assert np.array_equal(seen[r], global_image_from_state(orc.get_state(), env.goals, PLAIN).astype(np.uint8)), r
        orc.step_autoreset(tape[r], "next_step")
    assert np.array_equal(img.cpu().numpy(), seen[-1])
    lockstep.same_state(env.get_state(), orc.get_state())
    env.close()
