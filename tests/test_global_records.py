"""rw_global_records / rw_global_image_gather: the critic's global state kept as one byte record per env, and minibatches of global
images gathered from such records by a device index and expanded in one launch — the kernels (csrc/rware_global_state.h),
Engine.global_records / global_image_gather and WarehouseVecEnv.global_records_device / global_image_from_records.

  - CPU suite: the product sources on host threads (tests/emu; a device pointer is a host pointer there).
  - GPU suite (-m gpu): the same checks on the gfx950 library, then the torch surface and a captured loop.
Expectations never come from the code under test: the UNMODIFIED reference's own images (tests/golden/global_image), a numpy model of
the record format written here (record_model, from a get_state() dict), and the host form global_image_from_state, which
tests/test_oracle_vs_reference.py pins to the reference.  The gather is checked on numpy-built records, so it does not depend on the
record kernel.  Every comparison is exact equality of bit patterns (an image is integers 0 .. 4, exact in all four element types);
outputs lie in poisoned memory between two guards."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_util as gu
import lockstep
from device_backends import BACKENDS, GUARD, POISON
from models import ALL7, PLAIN
from rware_oracle import OracleVecEnv

import rware_amd
from rware_amd import _capi
from rware_amd.vector_env import global_image_from_state

P_ACT = [.05, .7, .1, .1, .05]
OK, INVALID, INDEX = _capi.RW_OK, _capi.RW_ERR_INVALID_ARG, _capi.RW_ERR_INDEX
ELEMS = {"float32": (_capi.GLOBAL_F32, 4), "uint8": (_capi.GLOBAL_U8, 1), "float16": (_capi.GLOBAL_F16, 2), "bfloat16": (_capi.GLOBAL_BF16, 2)}
SHIFTS = {"float32": (0, 4, 12), "uint8": (0, 1, 2, 4), "float16": (0, 2, 4), "bfloat16": (0, 2, 4)}   # bytes behind a 16-byte boundary
TINY = dict(shelf_columns=3, column_height=8, shelf_rows=1, n_agents=2)
LAYOUT_3x5 = "\n..x..\n.x.x.\n.g.g.\n"            # H = 3, W = 5: H*W + 1 = 16, a record without a spare byte ... plus its 15 zeros
LAYOUT_5x3 = "\n.x.\n...\n.x.\n...\ng.g\n"         # H = 5, W = 3: the other orientation


def rb_of(H, W):
    return (H * W + 1 + 15) & ~15


def bits(image, elem):
    """the bit patterns of a float32 image of small integers in the element type `elem`"""
    f = np.ascontiguousarray(image, np.float32)
    if elem == "float32":
        return f.view(np.uint32)
    if elem == "uint8":
        return f.astype(np.uint8)
    if elem == "float16":
        return f.astype(np.float16).view(np.uint16)
    assert not (f.view(np.uint32) & 0xFFFF).any()          # bfloat16: the upper half of a float32 that has no lower half
    return (f.view(np.uint32) >> 16).astype(np.uint16)


def record_model(st, goals):
    """The published record format (include/rware_hip_global_state.h) from a get_state() dict: uint8 (B, RB)."""
    grid = np.asarray(st["grid"])
    B, _, H, W = grid.shape
    code = np.zeros((B, H, W), np.uint8)
    code[grid[:, 1] > 0] |= 1
    q = np.asarray(st["queue"])
    for k in range(q.shape[1]):
        code[(grid[:, 1] == q[:, k, None, None]) & (q[:, k, None, None] > 0)] |= 2
    code[grid[:, 0] > 0] |= 4
    for gx, gy in goals:
        code[:, gy, gx] |= 8
    flags = np.zeros(B, np.uint8)
    mirrored = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for i in range(st["agent_x"].shape[1]):                # agent order: the highest index wins the direction of a shared cell
            x, y, carrying = int(st["agent_x"][b, i]), int(st["agent_y"][b, i]), st["agent_carry"][b, i] > 0
            if x < H and y < W:
                mirrored[b, x, y] = (mirrored[b, x, y] & 0x10) | (int(st["agent_dir"][b, i]) + 1) << 5 | (0x10 if carrying else 0)
            else:
                flags[b] |= 1 | (2 if carrying else 0)
    rec = np.zeros((B, rb_of(H, W)), np.uint8)
    rec[:, :H * W] = (code | mirrored).reshape(B, H * W)
    rec[:, H * W] = flags
    return rec


def lenient_plane(st, layer):
    """AGENT_DIRECTION / AGENT_LOAD as the reference writes them (`layer[ag.x, ag.y]`, the last agent winning), except that an agent
    outside the transposed bounds writes nothing — what the kernels leave where the reference raises"""
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
    """the host form, the transposed planes without the agents that make it raise: float32 (B, C', H', W')"""
    planes = [lenient_plane(st, l) if l in (3, 4) else global_image_from_state(st, goals, [l])[:, 0] for l in layers]
    img = np.stack(planes, axis=1)
    whole, raised = lockstep.attempt(lambda: global_image_from_state(st, goals, layers))
    assert raised or np.array_equal(whole, img)
    if pad is not None:
        d = [p - s for p, s in zip(pad, img.shape[1:])]
        img = np.pad(img, ((0, 0),) + tuple((k // 2, k - k // 2) for k in d))
    return img


class Output:
    """a poisoned device array with a guard on either side of `nbytes` bytes, the payload `shift` bytes behind a 16-byte boundary"""

    def __init__(self, be, nbytes, shift=0):
        self.lo, self.n = GUARD + shift, nbytes
        self.keep, base, self.read = be.alloc(self.lo + nbytes + GUARD)
        assert base % 16 == 0
        self.ptr = base + self.lo

    def payload(self, what):
        raw = self.read()
        assert (raw[:self.lo] == POISON).all() and (raw[self.lo + self.n:] == POISON).all(), f"{what}: a guard was written"
        return raw[self.lo:self.lo + self.n]

    def untouched(self, what):
        assert (self.read() == POISON).all(), f"{what}: something was written"


def status(eng):
    """what the next rw_sync returns; the status word is clear afterwards"""
    rc = eng.lib.rw_sync(eng._h)
    assert eng.lib.rw_sync(eng._h) == OK
    return rc


def device_records(be, eng, what="records"):
    """rw_global_records into a poisoned array -> uint8 (B, RB); it never touches the status word"""
    rb = eng.global_record_bytes
    assert rb == rb_of(eng.H, eng.W)
    out = Output(be, eng.B * rb)
    eng.global_records(out.ptr)
    assert status(eng) == OK, what
    return out.payload(what).reshape(eng.B, rb).copy()


def gather(be, eng, rec_ptr, n_records, index, layers, pad=None, elem="float32", wide=False, shift=0, what=None):
    """rw_global_image_gather into a poisoned array -> (bit patterns (n, C', H', W'), what the following rw_sync returned)"""
    code, size = ELEMS[elem]
    n = n_records if index is None else len(index)
    shape = (n,) + (tuple(pad) if pad is not None else (len(layers), eng.H, eng.W))
    out = Output(be, int(np.prod(shape)) * size, shift)
    i_ptr = 0 if index is None else be.ptr((index if len(index) else np.zeros(1)).astype(np.int64 if wide else np.int32))
    eng.global_image_gather(rec_ptr, n_records, i_ptr, n, layers, out.ptr, pad, code, wide)
    rc = status(eng)
    if n == 0:
        out.untouched(what)
        return np.zeros(shape, {4: np.uint32, 2: np.uint16, 1: np.uint8}[size]), rc
    return out.payload(what).view({4: np.uint32, 2: np.uint16, 1: np.uint8}[size]).reshape(shape).copy(), rc


def same(got, want_bits, what):
    if not np.array_equal(got, want_bits):
        bad = np.argwhere(got != want_bits)[:5]
        raise AssertionError(f"{what}: differs at {bad.tolist()}: got {[hex(got[tuple(b)]) for b in bad]}, want {[hex(want_bits[tuple(b)]) for b in bad]}")


# ------------------------------------------------------------------------------------------------ 1. the reference's own images
FIXTURE = os.path.join(gu.GOLDEN_DIR, "global_image", "global_image.npz")
REPLAYS = {"img-square-all7-msg1": [ALL7], "layoutstr-3ag": [ALL7], "tiny-2ag": [PLAIN, [3], [4]]}   # as tests/test_global_image.py


@pytest.fixture(scope="module")
def golden_images():
    z = np.load(FIXTURE, allow_pickle=False)
    return {k: z[k] for k in z.files if k != "meta"}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(REPLAYS))
def test_a_tape_of_records_gathered_in_shuffled_order_gives_the_images_of_the_reference(name, backend, golden_images):
    """one record per step into a (T, E, RB) tape, then the tape gathered in a shuffled order: the reference's image of every step
    where it did not raise, the lenient planes where it did, RW_ERR_INDEX exactly when a gathered step raised for a requested layer"""
    be = backend()
    meta, z = gu.load_fixture(name)
    E, T = meta["E"], meta["T"]
    env = rware_amd.WarehouseVecEnv(E, library=be.library(), **dict(gu.ctor_kwargs(meta), **be.kw))
    eng = env.engines[0]
    rb = eng.global_record_bytes
    env.reset(seed=meta["seed"])
    tape = Output(be, T * E * rb)
    states = []
    for t in range(T):
        _, rew, done, _, _ = env.step(z["actions"][t].astype(np.int32))
        assert np.array_equal(rew, z["rewards"][t]) and np.array_equal(done.astype(np.uint8), z["done"][t]), t
        eng.global_records(tape.ptr + t * E * rb)                  # (every slot of the tape is 16-byte aligned: RB is a multiple of 16)
        if name == "tiny-2ag":
            states.append(env.get_state())
    assert status(eng) == OK                                       # records never raise, whatever the agents did
    tape.payload(name)                                             # the guards around the tape
    rng = np.random.default_rng(17)
    for k, ls in enumerate(REPLAYS[name]):
        key = name + "/" + "-".join(map(str, ls))
        want, raised = golden_images[key + "/image"], golden_images[key + "/raised"].any(axis=1)
        assert want.shape == (T, E, len(ls), eng.H, eng.W)
        clean, raising = np.flatnonzero(~raised), np.flatnonzero(raised)
        if name == "tiny-2ag" and ls in ([3], [4]):
            assert len(clean) > 100 and len(raising) > 100, "the fixture has to hold both kinds of step"
        else:
            assert len(raising) == 0
        for steps, want_rc in ((clean, OK), (raising, INDEX)):
            if not len(steps):
                continue
            index = rng.permutation((steps[:, None] * E + np.arange(E)).ravel())          # every env of those steps, shuffled
            # (two element types per list, all four over a replay; the 2600-record tape takes one per call)
            elems = (("float32", "uint8", "float16", "bfloat16")[k % 4], ("bfloat16", "float16", "uint8", "float32")[k % 4])
            for elem in elems[:1 if name == "tiny-2ag" else 2] if want_rc == OK else elems[1:]:
                got, rc = gather(be, eng, tape.ptr, T * E, index, ls, elem=elem, wide=elem in ("uint8", "float16"), what=key)
                assert rc == want_rc, (key, elem, rc)
                if want_rc == OK:
                    exp = want.reshape(T * E, len(ls), eng.H, eng.W)[index]
                else:                                                                     # (single-layer lists: the lenient plane itself)
                    exp = np.stack([lenient_plane(states[i // E], ls[0])[i % E] for i in index])[:, None]
                    ok_envs = ~golden_images[key + "/raised"].reshape(T * E)[index].astype(bool)
                    assert np.array_equal(exp[ok_envs], want.reshape(T * E, 1, eng.H, eng.W)[index][ok_envs])
                same(got, bits(exp, elem), (key, elem))
    env.close()


# ------------------------------------------------------------------------------------------------ 2. records against the numpy model
# name -> (B, constructor keywords, (H, W), an oracle exists)
RECORD_SHAPES = {
    "tiny-7": (7, TINY, (11, 10), True),                                                            # H*W + 1 = 111: just below 7 * 16; H > W
    "wide-4x16": (5, dict(shelf_columns=5, column_height=1, shelf_rows=1, n_agents=3), (4, 16), True),   # 65: just above 4 * 16; W > H
    "layout-3x5": (1, dict(shelf_columns=0, column_height=0, shelf_rows=0, n_agents=2, request_queue_size=1, layout=LAYOUT_3x5), (3, 5), True),   # 16: no spare byte
    "layout-5x3": (5, dict(shelf_columns=0, column_height=0, shelf_rows=0, n_agents=2, request_queue_size=1, layout=LAYOUT_5x3), (5, 3), True),
    "29x28-10ag-5": (5, dict(shelf_columns=9, column_height=8, shelf_rows=3, n_agents=10), (29, 28), True),   # > 255 shelves: uint16 shadow
    "29x28-10ag-7": (7, dict(shelf_columns=9, column_height=8, shelf_rows=3, n_agents=10), (29, 28), True),   # 5 envs a workgroup: the last is ragged
    "tiny-65ag": (5, dict(TINY, n_agents=65, request_queue_size=20), (11, 10), False),              # > 64 agents (the oracle holds 64)
}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", list(RECORD_SHAPES))
def test_records_equal_the_numpy_model_byte_for_byte(shape, backend):
    """code bytes, flags and the zero tail, after the reset, through 12 steps and a masked reset"""
    be = backend()
    B, kw, grid, has_oracle = RECORD_SHAPES[shape]
    kw = lockstep.oracle_kwargs(None, max_steps=30, **kw)
    geom = be.kw if has_oracle or be.gpu else dict(jit="off")           # (65 agents: the engine's own geometry, the 64-thread one is too small)
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), **dict(kw, **geom))
    orc = OracleVecEnv(B, **kw) if has_oracle else None
    eng = env.engines[0]
    assert (eng.H, eng.W) == grid and eng.global_record_bytes == rb_of(*grid) == env.global_record_bytes
    assert (eng.S > 255) == shape.startswith("29x28")
    obs = env.reset(seed=11)[0]
    if orc:
        lockstep.same_obs(obs, orc.reset(seed=11), "reset obs")
    rng = np.random.default_rng(5)
    flagged = 0
    for t in range(13):
        if t == 7:
            m = (np.arange(B) % 2 == 0).astype(np.uint8)
            obs = env.reset(seed=77, mask=m)[0]
            if orc:
                lockstep.same_obs(obs, orc.reset(seed=77, mask=m), "masked reset obs", t)
        elif t:
            a = rng.choice(5, size=(B, env.n_agents), p=P_ACT).astype(np.int32)
            obs = env.step(a)[0]
            if orc:
                lockstep.same_obs(obs, orc.step_autoreset(a, "next_step")[0], "obs", t)
        st = orc.get_state() if orc else env.get_state()
        want = record_model(st, env.goals)
        got = device_records(be, eng, (shape, t))
        same(got, want, (shape, t))
        assert not got[:, grid[0] * grid[1] + 1:].any()
        flagged += int((want[:, grid[0] * grid[1]] != 0).sum())
    if shape in ("tiny-7", "wide-4x16", "tiny-65ag"):
        assert flagged > 0, "no state of this run left the transposed bounds"
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_two_agents_on_one_mirrored_cell_and_a_carried_requested_shelf(backend):
    be = backend()
    B = 3
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), n_agents=3, **dict(
        {k: v for k, v in rware_amd.env_kwargs("rware-tiny-2ag-v1").items() if k != "n_agents"}, **be.kw))
    env.reset(seed=2)
    st = env.get_state()
    H, W = env.grid_size
    ys, xs = np.nonzero(st["grid"][0, 1])
    y, x = int(ys[0]), int(xs[0])                          # a cell with a shelf, inside the transposed bounds
    assert x < H and y < W
    shelf = st["grid"][:, 1, y, x].copy()
    ax, ay, ad, ac, q = (st[k].copy() for k in ("agent_x", "agent_y", "agent_dir", "agent_carry", "queue"))
    ax[:, :2], ay[:, :2] = x, y                            # agents 0 and 1 share the cell; agent 2 stands in the bottom row: no mirrored cell
    ax[:, 2], ay[:, 2] = 0, H - 1
    ad[:, 0], ad[:, 1], ad[:, 2] = 3, 1, 0
    ac[:] = 0
    ac[0, 1], ac[1, 0] = shelf[0], shelf[1]                # env 0: the higher index carries, env 1: the lower one, env 2: nobody
    q[:, 0] = shelf                                        # ... and the carried shelf is a requested one
    q[:, 1] = np.where(q[:, 1] == shelf, shelf % env.n_shelves + 1, q[:, 1])
    env.set_state(agent_x=ax, agent_y=ay, agent_dir=ad, agent_carry=ac, queue=q)
    st = env.get_state()
    got = device_records(be, env.engines[0])
    same(got, record_model(st, env.goals), "injected")
    assert (got[:, x * W + y] >> 5 == 2).all(), "AGENT_DIRECTION: the highest agent index wins the shared (mirrored) cell"
    assert ((got[:, x * W + y] >> 4) & 1).tolist() == [1, 1, 0]
    assert (got[:, y * W + x] & 7 == 7).all()              # shelf, requested, agent: the carried requested shelf lies under its carrier
    assert got[:, H * W].tolist() == [1, 1, 1]             # agent 2 has no mirrored cell and carries nothing
    ac[2, 2] = st["grid"][2, 1][st["grid"][2, 1] > 0][-1]  # ... until it carries a shelf
    env.set_state(agent_carry=ac)
    got = device_records(be, env.engines[0])
    same(got, record_model(env.get_state(), env.goals), "injected, loaded")
    assert got[:, H * W].tolist() == [1, 1, 3]
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_global_records_device_with_numpy_output_gathers_the_shards(backend):
    be = backend()
    B = 10
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1")
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), devices=[0, 0, 0], **dict(kw, **be.kw))
    orc = OracleVecEnv(B, **kw)
    assert [e.B for e in env.engines] == [4, 3, 3]
    env.reset(seed=8)
    orc.reset(seed=8)
    rng = np.random.default_rng(4)
    for t in range(6):
        a = rng.choice(5, size=(B, 2), p=P_ACT).astype(np.int32)
        env.step(a)
        orc.step_autoreset(a, "next_step")
        got = env.global_records_device()
        assert got.dtype == np.uint8 and got.shape == (B, env.global_record_bytes)
        same(got, record_model(orc.get_state(), env.goals), t)
    with pytest.raises(ValueError):
        env.global_records_device(out=np.zeros((B, env.global_record_bytes), np.uint8))      # `out` is a device tensor of output="torch" envs
    env.close()


# ------------------------------------------------------------------------------------------------ 3. the gather, from numpy-built records
@pytest.fixture(params=BACKENDS)
def played(request):
    """a tiny-2ag engine, and 13 numpy-built records of ANOTHER batch a few steps into its episodes — clean ones first, then those with
    a flag — with their state: (backend, env, engine, state, records, device pointer of the records)"""
    be = request.param()
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1")
    env = rware_amd.WarehouseVecEnv(2, library=be.library(), **dict(kw, **be.kw))
    env.reset(seed=1)
    orc = OracleVecEnv(40, **kw)
    orc.reset(seed=12)
    rng = np.random.default_rng(9)
    for _ in range(9):
        orc.step_autoreset(rng.choice(5, size=(40, 2), p=P_ACT).astype(np.int32), "next_step")
    st = orc.get_state()
    flags = record_model(st, env.goals)[:, 110]
    pick = np.concatenate([np.flatnonzero(flags == 0)[:9], np.flatnonzero(flags & 1)[:4]])
    assert len(pick) == 13
    st = {k: np.asarray(v)[pick].copy() for k, v in st.items() if k != "rng"}
    outside = int(np.flatnonzero(st["agent_y"][12] >= 10)[0])          # record 12: the agent in the bottom row carries a shelf
    st["agent_carry"][12, outside] = 1
    rec = record_model(st, env.goals)
    assert (rec[:9, 110] == 0).all() and (rec[9:12, 110] == 1).all() and rec[12, 110] == 3
    yield be, env, env.engines[0], st, rec, be.ptr(rec)
    env.close()


LISTS = [(ALL7, None), ([0, 0, 6], None), ([0, 1, 2, 5, 6, 0, 1, 2], None), ([6, 2, 0], (4, 12, 13)), (ALL7, (8, 14, 11)), ([5] * 8, None)]


def test_gathered_images_equal_the_host_form_in_every_element_type_and_at_every_offset(played):
    """the nine clean records: every layer list and padding (an odd difference on each axis), element type and output offset; no index,
    reversed, repeats; both index widths"""
    be, env, eng, st, rec, r_ptr = played
    n_clean = 9
    patterns = {"identity": None, "reversed": np.arange(n_clean)[::-1].copy(), "repeats": np.array([4, 4, 0, 8, 4, 1, 1, 7, 3, 3, 3, 8, 0])}
    clean = {k: v[:n_clean] for k, v in st.items()}
    k = 0
    for layers, pad in LISTS:
        want = want_image(clean, env.goals, layers, pad)
        for elem in ELEMS:
            for kind, index in patterns.items():
                for wide in ((False,) if index is None else (False, True)):
                    shift = SHIFTS[elem][k % len(SHIFTS[elem])]
                    k += 1
                    what = (layers, pad, elem, kind, wide, shift)
                    got, rc = gather(be, eng, r_ptr, n_clean, index, layers, pad, elem, wide, shift, what)
                    assert rc == OK, what
                    same(got, bits(want if index is None else want[index], elem), what)
    for elem in ELEMS:                                      # every offset the element allows, on the list that has every layer
        want = want_image(clean, env.goals, ALL7, (7, 11, 13))
        for shift in SHIFTS[elem] + tuple(s for s in (6, 8, 15) if s % ELEMS[elem][1] == 0):
            got, rc = gather(be, eng, r_ptr, n_clean, patterns["repeats"], ALL7, (7, 11, 13), elem, True, shift, (elem, shift))
            assert rc == OK
            same(got, bits(want[patterns["repeats"]], elem), (elem, shift))


def test_the_flags_of_the_gathered_records_alone_decide_on_the_index_error(played):
    """records 9 .. 11: an agent without a mirrored cell; record 12: a carrying one.  RW_ERR_INDEX when such a record is GATHERED and
    its layer is asked for; the image is the lenient one"""
    be, env, eng, st, rec, r_ptr = played
    cases = [([3], [0, 5, 8], OK), ([3], [0, 9], INDEX), ([4], [9, 10, 11, 2], OK), ([4], [12], INDEX), ([3], [12], INDEX),
             (PLAIN, [9, 10, 11, 12], OK), (ALL7, [1, 12, 2], INDEX), ([4, 3], None, INDEX), ([0, 6], None, OK)]
    for k, (layers, index, want_rc) in enumerate(cases):
        index = None if index is None else np.array(index)
        elem = list(ELEMS)[k % 4]
        got, rc = gather(be, eng, r_ptr, 13, index, layers, elem=elem, wide=bool(k & 1), what=(layers, index))
        assert rc == want_rc, (layers, index, rc)
        want = want_image(st, env.goals, layers)
        same(got, bits(want if index is None else want[index], elem), (layers, index))


def test_an_index_out_of_range_gives_an_image_of_zeros_and_shows_at_sync(played):
    be, env, eng, st, rec, r_ptr = played
    want = want_image(st, env.goals, ALL7)
    for wide in (False, True):
        for elem in ELEMS:
            index = np.array([2, -1, 0, 9, 1, 7, 9 + 4 * wide])      # 9 records: -1 and n_records (int64: beyond them) are out of range
            got, rc = gather(be, eng, r_ptr, 9, index, ALL7, elem=elem, wide=wide, shift=SHIFTS[elem][1], what=(elem, wide))
            assert rc == INVALID, (elem, wide, rc)                    # (and the status is clear afterwards: status())
            bad = (index < 0) | (index >= 9)
            assert bad.sum() == 3 and not got[bad].any(), "an image of zeros, ACCESSIBLE included"
            same(got[~bad], bits(want[index[~bad]], elem), (elem, wide))
    got, rc = gather(be, eng, r_ptr, 9, np.array([1 << 40, -(1 << 40), 3]), [6], wide=True)       # nothing is read out of bounds
    assert rc == INVALID and not got[:2].any()
    same(got[2:], bits(want[3:4, 6:7], "float32"), "the good one")
    got, rc = gather(be, eng, r_ptr, 9, np.zeros(0, np.int64), ALL7, wide=True, what="empty")    # an empty index: RW_OK, nothing written
    assert rc == OK and got.shape[0] == 0


# ------------------------------------------------------------------------------------------------ 4. every refusal
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_entry_points_check_their_arguments(backend):
    be = backend()
    env = rware_amd.WarehouseVecEnv(6, library=be.library(), **dict(rware_amd.env_kwargs("rware-tiny-2ag-v1"), **be.kw))
    eng = env.engines[0]
    env.reset(seed=1)
    rb = eng.global_record_bytes
    assert eng.lib.rw_global_record_bytes(eng._h) == rb == 112 and eng.lib.rw_global_record_bytes(None) == INVALID
    vp = lambda p: C.c_void_p(int(p))
    i32x = lambda *v: (C.c_int32 * len(v))(*v)
    recs, out = Output(be, 6 * rb + 16), Output(be, 6 * 8 * 16 * 16 * 4 + 16)
    index = be.ptr(np.arange(8, dtype=np.int64))
    records, gather_ = eng.lib.rw_global_records, eng.lib.rw_global_image_gather
    assert records(None, vp(recs.ptr)) == INVALID and records(eng._h, None) == INVALID
    for off in (1, 4, 8):
        assert records(eng._h, vp(recs.ptr + off)) == INVALID, off                            # records_dev: 16-byte aligned
    good = i32x(0, 5)
    ok = dict(eng=eng._h, rec=vp(recs.ptr), n_rec=6, idx=vp(index), n_idx=4, layers=good, n_layers=2, pad=None, elem=0, flags=1, out=vp(out.ptr))
    call = lambda **kw: gather_(*dict(ok, **kw).values())
    refusals = {
        "a NULL engine": dict(eng=None), "NULL records": dict(rec=None), "NULL layers": dict(layers=None), "NULL out": dict(out=None),
        "negative n_records": dict(n_rec=-1), "negative n_index": dict(n_idx=-1),
        "a NULL index with unequal counts": dict(idx=None, n_idx=4), "an unknown elem": dict(elem=4), "a negative elem": dict(elem=-1),
        "unknown flag bits": dict(flags=2), "more unknown flag bits": dict(flags=1 | 8),
        "no layers": dict(n_layers=0), "nine layers": dict(layers=i32x(*[0] * 9), n_layers=9),
        "a layer above 6": dict(layers=i32x(0, 7)), "a negative layer": dict(layers=i32x(-1), n_layers=1),
        "a pad smaller in C": dict(pad=i32x(1, 11, 10)), "a pad smaller in H": dict(pad=i32x(2, 10, 10)), "a pad smaller in W": dict(pad=i32x(2, 11, 9)),
        "misaligned records": dict(rec=vp(recs.ptr + 8)), "a misaligned int64 index": dict(idx=vp(index + 4)),
        "a misaligned int32 index": dict(idx=vp(index + 2), flags=0), "a misaligned float32 out": dict(out=vp(out.ptr + 2)),
        "a misaligned float16 out": dict(out=vp(out.ptr + 1), elem=2), "a misaligned bfloat16 out": dict(out=vp(out.ptr + 3), elem=3),
        "2^35 elements per image": dict(pad=i32x(8, 65536, 65536), elem=1), "2^31 images": dict(n_idx=1 << 31, n_rec=1 << 31, idx=None),
        "2^52 bytes of records": dict(n_rec=1 << 50),
    }
    for what, kw in refusals.items():
        assert call(**kw) == INVALID, what
    assert "more than one launch holds" in eng.lib.rw_last_error(eng._h).decode()
    assert status(eng) == OK
    recs.untouched("refused calls")
    out.untouched("refused calls")
    assert call(n_idx=0) == OK and call(n_idx=0, idx=None, n_rec=0) == OK                     # nothing to gather: RW_OK, nothing written
    out.untouched("n_index == 0")
    assert records(eng._h, vp(recs.ptr)) == OK and call() == OK and call(idx=None, n_idx=6, flags=0) == OK
    assert call(out=vp(out.ptr + 1), elem=1) == OK and call(out=vp(out.ptr + 2), elem=3) == OK   # aligned to the element only
    assert status(eng) == OK
    with pytest.raises(_capi.EngineError):
        eng.global_image_gather(recs.ptr, 6, 0, 6, [0, 9], out.ptr)
    env.close()


# ------------------------------------------------------------------------------------------------ 5. the Python surface
def test_the_method_refuses_what_it_cannot_gather():
    """argument errors of global_image_from_records, raised before anything reaches the engine (host tensors serve)"""
    import torch
    from device_backends import GENERIC, emu_library

    env = rware_amd.WarehouseVecEnv(4, library=emu_library(), **dict(rware_amd.env_kwargs("rware-tiny-2ag-v1"), **GENERIC))
    rb = env.global_record_bytes
    good = torch.zeros((3, 4, rb), dtype=torch.uint8)
    idx = torch.arange(6)
    bad = {
        "a host tensor": dict(records=good), "a host tensor with an index": dict(records=good, index=idx),
        "a numpy array": dict(records=np.zeros((4, rb), np.uint8)), "a wrong last dimension": dict(records=torch.zeros((4, rb + 16), dtype=torch.uint8)),
        "int32 records": dict(records=torch.zeros((4, rb), dtype=torch.int32)),
        "a sliced input": dict(records=torch.zeros((4, 2 * rb), dtype=torch.uint8)[..., :rb]),
        "a float index": dict(records=good, index=idx.to(torch.float32)), "a 2-D index": dict(records=good, index=idx.reshape(2, 3)),
        "an unknown dtype": dict(records=good, dtype="float64"), "an unknown torch dtype": dict(records=good, dtype=torch.int8),
        "an unknown layer": dict(records=good, image_layers=[0, 7]), "no layer": dict(records=good, image_layers=[]),
        "out of the wrong shape": dict(records=good, index=idx[:4], out=torch.zeros((6, 2, 11, 10))),
        "out of the wrong dtype": dict(records=good, dtype="bfloat16", out=torch.zeros((12, 2, 11, 10), dtype=torch.float16)),
        "out on another device": dict(records=good, out=torch.zeros((12, 2, 11, 10), device="meta")),
        "a non-contiguous out": dict(records=good, out=torch.zeros((12, 2, 11, 20))[..., :10]),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            env.global_image_from_records(**kw)
            pytest.fail(f"{what}: accepted")
    with pytest.raises(AssertionError):
        env.global_image_from_records(good, pad_to_shape=(2, 10, 10))
    env.close()


@pytest.mark.gpu
def test_torch_records_and_images_are_cached_cuda_tensors_equal_to_the_host_form():
    import torch

    B, T = 16, 5
    env = rware_amd.WarehouseVecEnv(B, output="torch", **rware_amd.env_kwargs("rware-small-4ag-v1"))
    env.reset(seed=4)
    rb = env.global_record_bytes
    assert rb == rb_of(20, 10) == 208
    rng = np.random.default_rng(1)
    tape = torch.full((T, B, rb), 0xA5, dtype=torch.uint8, device="cuda")
    states = []
    for t in range(T):
        env.step(rng.choice(5, size=(B, 4), p=P_ACT).astype(np.int32))
        rec = env.global_records_device()
        assert rec.is_cuda and rec.dtype == torch.uint8 and tuple(rec.shape) == (B, rb)
        assert env.global_records_device() is rec                                   # allocated once
        assert env.global_records_device(out=tape[t]) is not rec
        env.sync()
        states.append(env.get_state())
        want = record_model(states[-1], env.goals)
        assert np.array_equal(rec.cpu().numpy(), want) and np.array_equal(tape[t].cpu().numpy(), want)
    st = {k: np.concatenate([s[k] for s in states]) for k in states[0] if k != "rng"}
    idx = torch.from_numpy(np.random.default_rng(2).integers(0, T * B, size=24)).cuda()
    pad = (6, 21, 12)
    want = want_image(st, env.goals, PLAIN, pad)[idx.cpu().numpy()]
    views = {torch.float32: torch.int32, torch.uint8: torch.uint8, torch.float16: torch.int16, torch.bfloat16: torch.int16}
    for dtype, tdt in (("float32", torch.float32), ("uint8", torch.uint8), ("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        a = env.global_image_from_records(tape, index=idx.to(torch.int32), image_layers=PLAIN, pad_to_shape=pad, dtype=dtype)
        env.sync()
        assert a.is_cuda and a.dtype == tdt and tuple(a.shape) == (24,) + pad
        assert torch.equal(a.view(views[tdt]), torch.from_numpy(want).to(tdt).cuda().view(views[tdt]))
        b = env.global_image_from_records(tape, index=idx, image_layers=PLAIN, pad_to_shape=pad, dtype=tdt)   # the same shape again
        assert b is a and b.data_ptr() == a.data_ptr()
    whole = env.global_image_from_records(tape)                                   # no index: every record of the tape, the default layers
    env.sync()
    assert tuple(whole.shape) == (T * B, 2, 20, 10) and np.array_equal(whole.cpu().numpy(), want_image(st, env.goals, [0, 5]))
    big = torch.zeros(24 * 5 * 200 + 8, dtype=torch.float16, device="cuda")
    out = big[1:1 + 24 * 5 * 200].view(24, 5, 20, 10)                              # 2 bytes behind a 16-byte boundary
    assert env.global_image_from_records(tape, idx, PLAIN, dtype=torch.float16, out=out) is out
    env.sync()
    assert np.array_equal(out.cpu().numpy(), want_image(st, env.goals, PLAIN)[idx.cpu().numpy()].astype(np.float16))
    assert big[0] == 0 and (big[1 + 24 * 5 * 200:] == 0).all()
    for bad in (dict(out=out[:-1]), dict(out=out.to(torch.uint8)), dict(out=out.cpu()), dict(out=out.transpose(2, 3)), dict(index=idx.cpu()),
                dict(records=tape.cpu(), index=idx.cpu())):
        with pytest.raises(ValueError):
            env.global_image_from_records(**dict(dict(records=tape, index=idx, image_layers=PLAIN, dtype=torch.float16), **bad))
    off = torch.zeros(B * rb + 16, dtype=torch.uint8, device="cuda")[8:8 + B * rb].view(B, rb)      # 8 bytes behind a 16-byte boundary
    for bad in (tape[0, :, :-16], tape[0].to(torch.int32), tape[0].cpu(), tape[0, :-1], off):
        with pytest.raises(ValueError):
            env.global_records_device(out=bad)
    env.global_image_from_records(tape, image_layers=[3])   # small is 20 x 10: after a few steps somebody stands at y >= 10
    with pytest.raises(IndexError):
        env.sync()
    env.global_image_from_records(tape, index=torch.tensor([0, T * B], device="cuda"))
    with pytest.raises(_capi.EngineError):
        env.sync()
    env.sync()
    env.close()


@pytest.mark.gpu
def test_a_tape_filled_inside_a_captured_loop_is_gathered_after_the_replays():
    import torch

    B, N, K = 16, 4, 3
    kw = lockstep.oracle_kwargs("rware-small-4ag-v1")
    env = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
    orc = OracleVecEnv(B, **kw)
    env.reset(seed=7)
    orc.reset(seed=7)
    rb = env.global_record_bytes
    actions = np.random.default_rng(6).choice(5, size=(2 * K, B, N), p=P_ACT).astype(np.int32)
    dev_actions = torch.from_numpy(actions).cuda()
    cursor = torch.zeros((), dtype=torch.long, device="cuda")
    tape = torch.zeros((K, B, rb), dtype=torch.uint8, device="cuda")            # one slot per step of the captured loop
    whole = torch.zeros((2 * K, B, rb), dtype=torch.uint8, device="cuda")
    calls = [0]

    def policy(obs, rewards, terminated):
        env.global_records_device(out=tape[calls[0] % K])                        # the state this round's observation describes, straight
        calls[0] += 1                                                            # into the tape: step k of the loop owns slot k
        a = dev_actions.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return a

    loop = env.capture_loop(policy, steps=K, warmup=0)
    assert calls[0] % K == 0
    cursor.zero_()
    tape.zero_()
    for r in range(2):
        loop.replay()
        torch.cuda.synchronize()                                                 # (the replay runs on the env's stream, the copy on torch's)
        whole[r * K:(r + 1) * K] = tape
        torch.cuda.synchronize()
    tape = whole
    states = []
    for r in range(2 * K):
        states.append(orc.get_state())
        assert np.array_equal(tape[r].cpu().numpy(), record_model(states[-1], env.goals)), r
        orc.step_autoreset(actions[r], "next_step")
    st = {k: np.concatenate([s[k] for s in states]) for k in states[0] if k != "rng"}
    idx = torch.from_numpy(np.random.default_rng(3).permutation(2 * K * B)).cuda()
    img = env.global_image_from_records(tape, idx, PLAIN, dtype="bfloat16")
    env.sync()
    assert torch.equal(img.view(torch.int16), torch.from_numpy(want_image(st, env.goals, PLAIN)[idx.cpu().numpy()]).to(torch.bfloat16).cuda().view(torch.int16))
    lockstep.same_state(env.get_state(), orc.get_state())
    env.close()
