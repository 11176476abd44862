"""rw_unpack_obs_gather: packed observation rows gathered by a device index array and unpacked, in one launch, into float32, float16 or
bfloat16 — the kernel (csrc/rware_minibatch.h), Engine.unpack_gather and WarehouseVecEnv.unpack_obs_device.

  - CPU suite: the product sources on host threads (tests/emu; a device pointer is a host pointer there).
  - GPU suite (-m gpu): the same checks on the gfx950 library, then the torch surface and a captured loop.
Expectations never come from the code under test: packed rows are rware_amd.pack_obs of random 0/1 bodies with chosen coordinates,
float32 is numpy's rware_amd.unpack_obs(packed[index]), float16 its .astype(np.float16), bfloat16 torch's CPU .to(torch.bfloat16); every
comparison is exact equality of bit patterns.  Outputs lie in poisoned memory between two guards (device_backends.alloc).
The engine does construct grids wider than 256 cells (H * W <= 10000): the 4 x 262 warehouse below has x coordinates 257 .. 261, which
bfloat16 cannot hold — ties to even both ways (257 -> 256, 259 -> 260) — and float16 can."""
import numpy as np
import pytest
import torch

import lockstep
from device_backends import BACKENDS, GUARD, POISON
from rware_oracle import OracleVecEnv

import rware_amd
from rware_amd import _capi

TINY = dict(shelf_columns=3, column_height=8, shelf_rows=1, n_agents=2)
# name -> (constructor keywords, L, PW, (H, W)): the smallest shapes at which the chunking can go wrong
ENGINES = {
    "L71": (dict(TINY, sensor_range=1), 71, 4, (11, 10)),                    # L % 8 = 7: every row straddles chunks in all three types
    "L80": (dict(TINY, sensor_range=1, msg_bits=1), 80, 4, (11, 10)),        # rows on chunk boundaries
    "L258": (dict(TINY, sensor_range=2, msg_bits=3), 258, 10, (11, 10)),     # L % 8 = 2: word-crossing nibbles
    "wide262": (dict(shelf_columns=87, column_height=1, shelf_rows=1, n_agents=2, sensor_range=1), 71, 4, (4, 262)),  # bfloat16 integer rounding
}
ELEMS = {"float32": (_capi.UNPACK_F32, 4), "float16": (_capi.UNPACK_F16, 2), "bfloat16": (_capi.UNPACK_BF16, 2)}
N_GROUPS = 7
CASES = [(name, norm) for name in ("L71", "L80", "L258") for norm in (False, True)] + [("wide262", False), ("wide262", True)]
OK, INVALID, UNSUPPORTED = _capi.RW_OK, _capi.RW_ERR_INVALID_ARG, _capi.RW_ERR_UNSUPPORTED


def make_env(be, name, norm=False, B=2, **more):
    kw = lockstep.oracle_kwargs(None, **ENGINES[name][0], normalised_coordinates=norm)
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), **dict(kw, **be.kw), **more)
    eng = env.engines[0]
    assert (eng.L, eng.PW, (eng.H, eng.W)) == ENGINES[name][1:], name
    return env, eng


def packed_rows(name, xy, seed):
    """uint32 (len(xy), PW): random 0/1 bodies behind the given cell coordinates, packed by rware_amd.pack_obs"""
    kw, L, PW, grid = ENGINES[name]
    rng = np.random.default_rng(seed)
    obs = rng.integers(0, 2, size=(len(xy), L)).astype(np.float32)
    obs[:, :2] = xy
    p = rware_amd.pack_obs(obs, grid, kw["sensor_range"], kw.get("msg_bits", 0))
    assert p.shape == (len(xy), PW) and p.dtype == np.uint32
    return p


def some_cells(name, n, seed):
    """n cells of the grid, (0, 0) and (W-1, H-1) among them, the rest random"""
    H, W = ENGINES[name][3]
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.integers(0, W, size=n), rng.integers(0, H, size=n)], axis=1)
    xy[0], xy[-1] = (0, 0), (W - 1, H - 1)
    xy[n // 2] = (W - 1, 0)
    return xy


def expected_bits(name, norm, packed, index, elem):
    """the bit patterns of unpack_obs(packed[index]).to(elem), formed on the host: (uint32 or uint16 array, float32 array)"""
    kw, L, PW, grid = ENGINES[name]
    f32 = rware_amd.unpack_obs(packed if index is None else packed[index], grid, kw["sensor_range"], kw.get("msg_bits", 0), norm)
    assert f32.dtype == np.float32
    if elem == "float32":
        return f32.view(np.uint32), f32
    if elem == "float16":
        with np.errstate(over="ignore"):
            return f32.astype(np.float16).view(np.uint16), f32
    return torch.from_numpy(f32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16), f32


def index_patterns(n_groups):
    """name -> int64 index array, or None for the identity (a NULL index)"""
    rng = np.random.default_rng(23)
    rand = rng.integers(0, n_groups, size=n_groups + 4)
    rand[1] = rand[0]
    return {"identity": None, "reversed": np.arange(n_groups)[::-1].copy(), "all-equal": np.full(n_groups, n_groups // 2),
            "random-repeats": rand, "one": np.array([n_groups - 1]), "none": np.zeros(0, np.int64)}


class Output:
    """a poisoned device array with a guard on either side of `count` elements of `size` bytes, the payload `offset_elems` elements
    behind a 16-byte boundary"""

    def __init__(self, be, count, size, offset_elems=0):
        self.lo, self.n = GUARD + offset_elems * size, count * size
        self.keep, base, self.read = be.alloc(self.lo + self.n + GUARD)
        assert base % 16 == 0
        self.ptr = base + self.lo

    def check(self, want_bits, what):
        raw = self.read()
        assert (raw[:self.lo] == POISON).all() and (raw[self.lo + self.n:] == POISON).all(), f"{what}: a guard was written"
        got = raw[self.lo:self.lo + self.n].view(want_bits.dtype).reshape(want_bits.shape)
        if not np.array_equal(got, want_bits):
            bad = np.argwhere(got != want_bits)[:5]
            raise AssertionError(f"{what}: differs at {bad.tolist()}: got {[hex(got[tuple(b)]) for b in bad]}, want {[hex(want_bits[tuple(b)]) for b in bad]}")

    def untouched(self, what):
        assert (self.read() == POISON).all(), f"{what}: something was written"


def index_ptr(be, index, wide):
    """(an empty index still gets a real array behind its pointer: NULL would mean the identity)"""
    return 0 if index is None else be.ptr((index if len(index) else np.zeros(1)).astype(np.int64 if wide else np.int32))


# ------------------------------------------------------------------------------------------------ 1. values, every pattern
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("name,norm", CASES)
def test_gathered_rows_equal_the_host_unpack_of_the_indexed_rows_bit_for_bit(name, norm, G, backend):
    """7 groups of G rows; every index pattern, element type, index width and output address (16-byte aligned, and one element behind
    such a boundary: the scalar path)"""
    be = backend()
    env, eng = make_env(be, name, norm)
    L = eng.L
    packed = packed_rows(name, some_cells(name, N_GROUPS * G, seed=G), seed=10 + G).reshape(N_GROUPS, G, eng.PW)
    p_ptr = be.ptr(packed)
    for kind, index in index_patterns(N_GROUPS).items():
        n = N_GROUPS if index is None else len(index)
        ptrs = {wide: index_ptr(be, index, wide) for wide in ((False,) if index is None else (False, True))}
        for elem, (code, size) in ELEMS.items():
            want, _ = expected_bits(name, norm, packed, index, elem)
            assert want.shape == (n, G, L)
            for wide, i_ptr in ptrs.items():
                for off in (0, 1):
                    what = f"{name} norm={norm} G={G} {kind} {elem} int{64 if wide else 32} offset {off}"
                    out = Output(be, n * G * L, size, off)
                    eng.unpack_gather(p_ptr, N_GROUPS, G, i_ptr, n, code, wide, out.ptr)
                    eng.sync()
                    if n == 0:
                        out.untouched(what)
                    else:
                        out.check(want, what)
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name,norm", CASES)
def test_every_cell_of_the_grid_in_every_element_type(name, norm, backend):
    """one row per cell, (0, 0) and (W-1, H-1) included, through the identity (a NULL index): the coordinates are the only elements the
    16-bit types round — normalised ones v / (dim - 1) in both, integers beyond 256 in bfloat16"""
    be = backend()
    env, eng = make_env(be, name, norm)
    H, W = eng.H, eng.W
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="ij"), axis=-1).reshape(-1, 2)
    assert len(xy) == H * W and tuple(xy[0]) == (0, 0) and tuple(xy[-1]) == (W - 1, H - 1)
    packed = packed_rows(name, xy, seed=4)
    p_ptr = be.ptr(packed)
    for elem, (code, size) in ELEMS.items():
        want, f32 = expected_bits(name, norm, packed, None, elem)
        out = Output(be, len(xy) * eng.L, size)
        eng.unpack_gather(p_ptr, len(xy), 1, 0, len(xy), code, False, out.ptr)
        eng.sync()
        out.check(want, f"{name} norm={norm} {elem}")
        if elem != "float32":                      # the case means something: some coordinate is inexact in this type
            exact = want[:, :2].view(np.float16).astype(np.float32) if elem == "float16" else \
                torch.from_numpy(want[:, :2].view(np.int16).copy()).view(torch.bfloat16).to(torch.float32).numpy()
            assert (exact != f32[:, :2]).any() == (norm or (name == "wide262" and elem == "bfloat16")), (name, norm, elem)
    env.close()


# ------------------------------------------------------------------------------------------------ 2. a bad index
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["L71", "L258"])
def test_a_bad_index_gives_a_group_of_zeros_and_one_invalid_arg_at_the_next_sync(name, backend):
    be = backend()
    env, eng = make_env(be, name)
    G, L = 2, eng.L
    packed = packed_rows(name, some_cells(name, N_GROUPS * G, seed=1), seed=2).reshape(N_GROUPS, G, eng.PW)
    p_ptr = be.ptr(packed)
    for bad, wide in ((-1, False), (N_GROUPS, False), (-1, True), (N_GROUPS, True), (2**31, True)):
        index = np.array([3, bad, 0, 6, bad, 5], np.int64)
        good = index != bad
        for elem, (code, size) in ELEMS.items():
            for off in (0, 1):
                what = f"{name} bad={bad} {elem} offset {off}"
                want, _ = expected_bits(name, False, packed, np.where(good, index, 0), elem)
                want = want.copy()
                want[~good] = 0
                out = Output(be, len(index) * G * L, size, off)
                eng.unpack_gather(p_ptr, N_GROUPS, G, index_ptr(be, index, wide), len(index), code, wide, out.ptr)
                assert eng.lib.rw_sync(eng._h) == INVALID, what
                assert b"rw_unpack_obs_gather" in eng.lib.rw_last_error(eng._h)
                assert eng.lib.rw_sync(eng._h) == OK, what
                out.check(want, what)
    # ... and a clean call afterwards leaves no flag behind
    out = Output(be, N_GROUPS * G * L, 4)
    eng.unpack_gather(p_ptr, N_GROUPS, G, 0, N_GROUPS, _capi.UNPACK_F32, False, out.ptr)
    assert eng.lib.rw_sync(eng._h) == OK
    env.close()


# ------------------------------------------------------------------------------------------------ 3. refusals
@pytest.mark.parametrize("backend", BACKENDS)
def test_each_refusal_returns_its_code_and_writes_nothing(backend):
    be = backend()
    env, eng = make_env(be, "L71")
    G, L = 2, eng.L
    packed = packed_rows("L71", some_cells("L71", N_GROUPS * G, seed=1), seed=2).reshape(N_GROUPS, G, eng.PW)
    p, i32, i64 = be.ptr(packed), be.ptr(np.arange(N_GROUPS, dtype=np.int32)), be.ptr(np.arange(N_GROUPS, dtype=np.int64))
    out = Output(be, N_GROUPS * G * L, 4)
    o = out.ptr
    fn, h = eng.lib.rw_unpack_obs_gather, eng._h
    F32, F16, BF16, I64 = _capi.UNPACK_F32, _capi.UNPACK_F16, _capi.UNPACK_BF16, _capi.UNPACK_INDEX64
    assert p % 16 == 0 and i32 % 8 == 0 and i64 % 8 == 0 and o % 16 == 0
    refused = {
        "NULL engine": (None, p, N_GROUPS, G, i32, N_GROUPS, F32, 0, o),
        "NULL packed_dev": (h, None, N_GROUPS, G, i32, N_GROUPS, F32, 0, o),
        "NULL out_dev": (h, p, N_GROUPS, G, i32, N_GROUPS, F32, 0, None),
        "negative n_groups": (h, p, -1, G, i32, N_GROUPS, F32, 0, o),
        "negative n_index": (h, p, N_GROUPS, G, i32, -1, F32, 0, o),
        "rows_per_group 0": (h, p, N_GROUPS, 0, i32, N_GROUPS, F32, 0, o),
        "rows_per_group -1": (h, p, N_GROUPS, -1, i32, N_GROUPS, F32, 0, o),
        "elem 3": (h, p, N_GROUPS, G, i32, N_GROUPS, 3, 0, o),
        "elem -1": (h, p, N_GROUPS, G, i32, N_GROUPS, -1, 0, o),
        "flag bit 2": (h, p, N_GROUPS, G, i32, N_GROUPS, F32, 2, o),
        "flag bits 1 | 4": (h, p, N_GROUPS, G, i64, N_GROUPS, F32, I64 | 4, o),
        "NULL index, n_index != n_groups": (h, p, N_GROUPS, G, None, N_GROUPS - 1, F32, 0, o),
        "NULL index, n_index 0": (h, p, N_GROUPS, G, None, 0, F32, 0, o),
        "packed_dev at 2 bytes": (h, p + 2, N_GROUPS - 1, G, i32, N_GROUPS, F32, 0, o),
        "int32 index at 2 bytes": (h, p, N_GROUPS, G, i32 + 2, N_GROUPS - 1, F32, 0, o),
        "int64 index at 4 bytes": (h, p, N_GROUPS, G, i64 + 4, N_GROUPS - 1, F32, I64, o),
        "float32 out at 2 bytes": (h, p, N_GROUPS, G, i32, N_GROUPS - 1, F32, 0, o + 2),
        "float16 out at 1 byte": (h, p, N_GROUPS, G, i32, N_GROUPS, F16, 0, o + 1),
        "bfloat16 out at 1 byte": (h, p, N_GROUPS, G, i32, N_GROUPS, BF16, 0, o + 1),
        "more than one launch holds": (h, p, N_GROUPS, G, i32, 2**45, F32, 0, o),
        "more than int64 holds": (h, p, N_GROUPS, 2**31 - 1, i32, 2**62, BF16, 0, o),
    }
    for what, args in refused.items():
        assert fn(*args) == INVALID, what
        assert what == "NULL engine" or eng.lib.rw_last_error(h), what
    assert eng.lib.rw_sync(h) == OK
    out.untouched("refusals")
    # n_index == 0 is a call that does nothing
    assert fn(h, p, N_GROUPS, G, i32, 0, F32, 0, o) == OK and fn(h, p, 0, G, None, 0, F16, 0, o) == OK
    assert eng.lib.rw_sync(h) == OK
    out.untouched("n_index 0")
    env.close()
    # an IMAGE engine has no packed rows
    kw = lockstep.oracle_kwargs(None, **TINY, observation_type=rware_amd.ObservationType.IMAGE)
    env = rware_amd.WarehouseVecEnv(2, library=be.library(), **dict(kw, **be.kw))
    h = env.engines[0]._h
    assert fn(h, p, N_GROUPS, G, i32, N_GROUPS, F32, 0, o) == UNSUPPORTED
    assert env.engines[0].lib.rw_sync(h) == OK
    out.untouched("IMAGE engine")
    env.close()


# ------------------------------------------------------------------------------------------------ 4. end to end, against the oracle
@pytest.mark.parametrize("backend", BACKENDS)
def test_minibatches_gathered_from_a_packed_rollout_tape_are_the_oracles_observations(backend):
    be = backend()
    B, T = 5, 3
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1")
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), obs_format="packed", **dict(kw, **be.kw))
    orc = OracleVecEnv(B, **kw)
    eng = env.engines[0]
    N, L, PW = eng.N, eng.L, eng.PW
    env.reset(seed=9)
    orc.reset(seed=9)
    rng = np.random.default_rng(5)
    actions = rng.choice(5, size=(T, B, N), p=[.05, .7, .1, .1, .05]).astype(np.int32)
    tape = np.asarray(env.rollout(actions)[0])
    assert tape.shape == (T, B, N, PW) and tape.dtype == np.uint32
    want = np.stack([orc.step_autoreset(actions[t], "next_step")[0] for t in range(T)]).reshape(T * B, N, L)
    index = rng.permutation(T * B)
    assert (index != np.arange(T * B)).any()
    p_ptr = be.ptr(tape.reshape(T * B, N, PW))
    for elem, (code, size) in ELEMS.items():
        for wide in (False, True):
            out = Output(be, T * B * N * L, size)
            eng.unpack_gather(p_ptr, T * B, N, index_ptr(be, index, wide), T * B, code, wide, out.ptr)
            env.sync()
            raw = out.read()[out.lo:out.lo + out.n]
            if elem == "float32":
                lockstep.same_obs(raw.view(np.float32).reshape(T * B, N, L), want[index], f"gathered {elem}")
            elif elem == "float16":
                lockstep.same_obs(raw.view(np.float16).reshape(T * B, N, L), want[index].astype(np.float16), f"gathered {elem}")
            else:
                lockstep.same_obs(raw.view(np.int16).reshape(T * B, N, L),
                                  torch.from_numpy(want[index]).to(torch.bfloat16).view(torch.int16).numpy(), f"gathered {elem}")
    env.close()


# ------------------------------------------------------------------------------------------------ 5. the Python method
def test_the_python_method_refuses_bad_arguments_with_value_error():
    """argument checks come before anything touches a device: host tensors reach every one of them here"""
    from device_backends import Host

    be = Host()
    env, eng = make_env(be, "L71", obs_format="packed")
    N, PW, L = eng.N, eng.PW, eng.L
    good = torch.zeros((6, N, PW), dtype=torch.int32)
    idx = torch.arange(6)
    bad = {
        "a host tensor": dict(packed=good),
        "a host tensor with an index": dict(packed=good, index=idx),
        "a numpy array": dict(packed=np.zeros((6, N, PW), np.uint32)),
        "a wrong last dimension": dict(packed=torch.zeros((6, N, PW + 1), dtype=torch.int32)),
        "rows without a leading dimension": dict(packed=torch.zeros((PW,), dtype=torch.int32)),
        "float rows": dict(packed=torch.zeros((6, N, PW), dtype=torch.float32)),
        "a non-contiguous input": dict(packed=torch.zeros((N, 6, PW), dtype=torch.int32).transpose(0, 1)),
        "a sliced input": dict(packed=torch.zeros((6, N, 2 * PW), dtype=torch.int32)[..., :PW]),
        "a float index": dict(packed=good, index=idx.to(torch.float32)),
        "a 2-D index": dict(packed=good, index=idx.reshape(2, 3)),
        "an unknown dtype": dict(packed=good, dtype="float64"),
        "an unknown torch dtype": dict(packed=good, dtype=torch.int8),
        "out of the wrong shape": dict(packed=good, index=idx[:4], out=torch.zeros((6, N, L))),
        "out of the wrong dtype": dict(packed=good, dtype="bfloat16", out=torch.zeros((6, N, L), dtype=torch.float16)),
        "out on another device": dict(packed=good, out=torch.zeros((6, N, L), device="meta")),
        "a non-contiguous out": dict(packed=good, out=torch.zeros((6, N, 2 * L))[..., :L]),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            env.unpack_obs_device(**kw)
            pytest.fail(f"{what}: accepted")
    env.close()


@pytest.mark.gpu
def test_unpack_obs_device_equals_the_torch_op_path_and_keeps_its_tensor():
    T = 4
    env = rware_amd.WarehouseVecEnv(6, output="torch", obs_format="packed", normalised_coordinates=True,
                                    **lockstep.oracle_kwargs("rware-tiny-2ag-v1"))
    B, N = env.num_envs, env.n_agents
    env.reset(seed=3)
    actions = torch.from_numpy(np.random.default_rng(1).choice(5, size=(T, B, N)).astype(np.int32)).cuda()
    tape = env.rollout(actions)[0]
    PW = tape.shape[-1]
    assert tuple(tape.shape) == (T, B, N, PW) and tape.dtype == torch.int32 and tape.is_cuda
    flat = tape.reshape(T * B, N, PW)
    idx = torch.from_numpy(np.random.default_rng(2).integers(0, T * B, size=40)).cuda()
    assert idx.dtype == torch.int64
    L = env.unpack_obs(flat[:1]).shape[-1]
    buf = torch.full((40, N, L), 7.0, dtype=torch.bfloat16, device="cuda")
    got = env.unpack_obs_device(flat, index=idx, dtype=torch.bfloat16, out=buf)
    env.sync()
    assert got is buf
    want = env.unpack_obs(flat[idx]).to(torch.bfloat16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    for dtype, tdt in (("float32", torch.float32), ("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        a = env.unpack_obs_device(flat, index=idx.to(torch.int32), dtype=dtype)
        env.sync()
        assert a.dtype == tdt and tuple(a.shape) == (40, N, L)
        assert torch.equal(a.view(torch.int32 if tdt == torch.float32 else torch.int16),
                           env.unpack_obs(flat[idx]).to(tdt).view(torch.int32 if tdt == torch.float32 else torch.int16))
        b = env.unpack_obs_device(flat, index=idx, dtype=tdt)                     # the same shapes again: nothing new is allocated
        assert b is a and b.data_ptr() == a.data_ptr()
    whole = env.unpack_obs_device(env.device_tensor("obs_packed"))               # the live rows, no index: the whole array
    env.sync()
    assert torch.equal(whole, env.unpack_obs(env.device_tensor("obs_packed")))
    with pytest.raises(ValueError):
        env.unpack_obs_device(flat.cpu(), index=idx.cpu())
    with pytest.raises(ValueError):
        env.unpack_obs_device(flat, index=idx.cpu())
    env.close()


@pytest.mark.gpu
def test_a_captured_call_follows_the_index_contents_at_every_replay():
    """one captured kernel and no parallel branches; a host synchronisation or an allocation inside the capture would fail it"""
    env = rware_amd.WarehouseVecEnv(8, output="torch", obs_format="packed", **lockstep.oracle_kwargs("rware-tiny-2ag-v1"))
    B, N = env.num_envs, env.n_agents
    env.reset(seed=4)
    packed = env.device_tensor("obs_packed")
    L = env.unpack_obs(packed[:1]).shape[-1]
    idx = torch.arange(3, dtype=torch.int64, device="cuda")
    out = torch.zeros((3, N, L), dtype=torch.float16, device="cuda")
    acts = torch.ones((B, N), dtype=torch.int32, device="cuda")

    def policy(obs, rew, term):
        env.unpack_obs_device(packed, index=idx, dtype="float16", out=out)
        return acts

    loop = env.capture_loop(policy, steps=1, warmup=1)
    for pick in ([7, 0, 7], [2, 5, 1]):
        idx.copy_(torch.tensor(pick, dtype=torch.int64, device="cuda"))
        before = env.unpack_obs(packed.clone())                                   # the rows the replay's policy call sees
        loop.replay()
        env.sync()
        assert torch.equal(out.view(torch.int16), before[torch.tensor(pick, device="cuda")].to(torch.float16).view(torch.int16)), pick
    env.close()
