"""The buffer kinds are described once on each side of the C boundary — the `kKinds` table of csrc/rware_capi.hip and `_capi.BUFFERS` —
and the two descriptions agree with include/rware_hip.h and with each other: for every name of the Python table, in engines built
with every opt-in output alone and all together, rw_get_buffer reports the table's shape where the kind exists with that
configuration and an empty buffer where it does not, and rw_write refuses exactly the read-only kinds.

  - CPU suite: the product sources on host threads (tests/emu);
  - GPU suite: the gfx950 library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rware_amd
from rware_amd import ObservationType, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rware_hip.h")

B = 7   # a ragged last workgroup
READ_ONLY = {"truncated", "obs_packed", "action_mask"}
# what a kind exists with: the construction switch that has to be on (the rest exists in every engine)
EXISTS_WITH = {"stat_deliveries": "stats", "stat_failed_moves": "stats", "ep_return": "episode_stats", "ep_length": "episode_stats",
               "ep_last_return": "episode_stats", "ep_last_length": "episode_stats", "ep_count": "episode_stats",
               "action_mask": "action_mask", "obs_packed": "packed", "final_obs": "same_step", "final_features": "same_step_dict"}
ALL_FOUR = dict(stats=True, episode_stats=True, action_mask=True, obs_format="packed")
ENGINES = [  # (constructor arguments, the switches of EXISTS_WITH that are on)
    (dict(), set()),
    (dict(stats=True), {"stats"}),
    (dict(episode_stats=True), {"episode_stats"}),
    (dict(action_mask=True), {"action_mask"}),
    (dict(obs_format="packed"), {"packed"}),
    (ALL_FOUR, {"stats", "episode_stats", "action_mask", "packed"}),
    (dict(autoreset_mode="same_step", observation_type=ObservationType.IMAGE_DICT), {"same_step", "same_step_dict"}),
]


def check_buffer_table(lib):
    kw = rware_amd.env_kwargs("rware-tiny-2ag-v1")
    for args, on in ENGINES:
        env = rware_amd.WarehouseVecEnv(B, library=lib, **dict(kw, **args))
        env.reset(seed=3)
        eng = env.engines[0]
        assert set(eng.shapes) == set(_capi.BUFFERS) == set(_capi.BUF) == set(_capi.BUF_DTYPE)
        for name, (kind, dtype, _, role) in _capi.BUFFERS.items():
            what = (sorted(on), name)
            exists = (name != "obs" or "packed" not in on) and EXISTS_WITH.get(name, None) in on | {None}
            ptr, nb = C.c_void_p(), C.c_size_t(7)
            assert eng.lib.rw_get_buffer(eng._h, kind, C.byref(ptr), C.byref(nb)) == _capi.RW_OK, what
            want = int(np.prod(eng.shapes[name])) * np.dtype(dtype).itemsize
            assert nb.value == (want if exists else 0) and (want > 0 or not exists), (what, nb.value, want)
            if name in ("obs", "obs_packed"):
                assert bool(ptr.value) == exists, what        # the observation format the engine does not produce: no pointer
            # rw_write with the buffer's own size (0 bytes for an empty one): refused for the read-only kinds, with and without their flag
            src = np.zeros(max(nb.value, 1), np.uint8)
            if name in READ_ONLY:
                assert eng.lib.rw_write(eng._h, kind, src.ctypes.data, nb.value) == _capi.RW_ERR_INVALID_ARG, what
                assert b"read-only" in eng.lib.rw_last_error(eng._h), what
                assert role == "io" and name not in _capi.WRITABLE_STATE
            elif not exists:
                assert eng.lib.rw_write(eng._h, kind, None, 0) == _capi.RW_OK, what
            else:                                             # (its own contents written back: the state does not move)
                eng.write(name, eng.read(name))
        env.close()


@pytest.mark.timeout(1500)
def test_emulated_every_buffer_kind_has_the_tables_size_in_every_configuration():
    from engine_backend import build_emu
    check_buffer_table(build_emu())


@pytest.mark.gpu
def test_every_buffer_kind_has_the_tables_size_in_every_configuration():
    check_buffer_table(None)


def test_python_table_matches_the_headers_enum():
    """enum rw_buffer_kind of include/rware_hip.h, parsed: the same names, the same values and RW_BUF_KIND_COUNT as _capi.BUFFERS."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"enum\s+rw_buffer_kind\s*\{(.*?)\}", src, flags=re.S).group(1)
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(RW_BUF_[A-Z_0-9]+)\s*=\s*(\d+)", body)}
    count = enum.pop("RW_BUF_KIND_COUNT")
    assert enum == {"RW_BUF_" + name.upper(): row[0] for name, row in _capi.BUFFERS.items()}
    assert count == len(_capi.BUFFERS) and sorted(enum.values()) == list(range(count))
    assert [row[0] for row in _capi.BUFFERS.values()] == list(range(count))   # (the table lists the kinds in the enum's order)
