"""The host-side models more than one test module compares an engine with, in plain numpy: the action-mask contract (pinned by
tests/test_action_mask.py), the episode-statistics contract (tests/test_episode_stats.py), two engines side by side."""
from collections import Counter

import numpy as np

PLAIN = [0, 1, 2, 5, 6]          # the layers that never raise
ALL7 = [0, 1, 2, 3, 4, 5, 6]
EPISODE_BUFFERS = ("return", "length", "last_return", "last_length", "count")


def mask_model(st, hw):
    """(byte (B, N) uint8, Counter of the cases met) — the definition at RW_ACTION_MASK_ON, from a get_state() dict and the highway array"""
    grid = st["grid"]
    B, _, H, W = grid.shape
    x, y, d, c = st["agent_x"], st["agent_y"], st["agent_dir"], st["agent_carry"] > 0
    tx = x + np.array([0, 0, -1, 1])[d]
    ty = y + np.array([-1, 1, 0, 0])[d]
    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    cx, cy, e = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1), np.arange(B)[:, None]
    occ = np.where(inside, grid[e, 0, cy, cx], 0)           # the agent standing on the cell ahead, 1-based
    shelf_t = np.where(inside, grid[e, 1, cy, cx], 0)
    occ_loaded = (occ > 0) & c[e, np.maximum(occ, 1) - 1]
    cancel = c & (shelf_t != 0) & ~occ_loaded               # rware/warehouse.py:829-844
    fwd = inside & ~cancel
    toggle = np.where(c, hw[y, x] == 0, grid[e, 1, y, x] != 0)   # :893-895, :889-892
    byte = (1 | 4 | 8 | ((fwd & (occ == 0)) << 1) | (toggle << 4) | ((fwd & (occ > 0)) << 5)).astype(np.uint8)
    met = Counter({"wall": int((~inside).sum()), "standing_shelf_while_loaded": int((inside & cancel & (occ == 0)).sum()),
                   "agent_ahead": int((fwd & (occ > 0)).sum()), "toggle_valid_unloaded": int((~c & toggle).sum()),
                   "toggle_invalid_unloaded": int((~c & ~toggle).sum()), "toggle_valid_loaded": int((c & toggle).sum()),
                   "toggle_invalid_loaded": int((c & ~toggle).sum())})
    return byte, met


def bits(byte, permissive=False):
    byte = np.asarray(byte)
    if permissive:
        byte = byte | ((byte >> 4) & 2)
    return ((byte[..., None] >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)


class EpisodeModel:
    """The five buffers, from (rewards, terminated) per step.  NEXT_STEP: the step after a `terminated` is a reset step."""

    def __init__(self, B, N, mode):
        self.mode = mode
        self.v = {"return": np.zeros((B, N), np.float32), "length": np.zeros(B, np.int32), "last_return": np.zeros((B, N), np.float32),
                  "last_length": np.zeros(B, np.int32), "count": np.zeros(B, np.int32)}
        self.pending = np.zeros(B, bool)

    def reset(self, mask=None):
        m = np.ones(len(self.pending), bool) if mask is None else np.asarray(mask, bool)
        self.v["return"][m] = 0
        self.v["length"][m] = 0
        self.pending[m] = False

    def step(self, rewards, terminated):
        v, rs = self.v, self.pending.copy()
        v["return"][rs] = 0                       # a reset step: cleared, nothing recorded
        v["length"][rs] = 0
        v["return"][~rs] += np.asarray(rewards, np.float32)[~rs]
        v["length"][~rs] += 1
        d = ~rs & np.asarray(terminated, bool)
        v["last_return"][d] = v["return"][d]
        v["last_length"][d] = v["length"][d]
        v["count"][d] += 1
        v["return"][d] = 0
        v["length"][d] = 0
        self.pending = d if self.mode == "next_step" else np.zeros_like(d)


def same_buffers(got, model, what):
    for k in EPISODE_BUFFERS:
        g, w = np.asarray(got[k]), model.v[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, what, g.dtype, g.shape)
        assert np.array_equal(g, w), (k, what, np.argwhere(g != w)[:5].tolist())


def everything(env):
    """every state field and every output / opt-in buffer the engine has, as host arrays"""
    eng = env.engines[0]
    out = dict(env.get_state())
    names = [eng.obs_name, "rewards", "terminated", "truncated", "need_reset", "features"]
    names += ["action_mask"] * eng.action_mask + ["stat_deliveries", "stat_failed_moves"] * eng.stats
    for n in names:
        out["buf:" + n] = eng.read(n)
    return out


def same_everything(a, b, what):
    ea, eb = everything(a), everything(b)
    assert ea.keys() == eb.keys()
    for k in ea:
        assert ea[k].dtype == eb[k].dtype and np.array_equal(ea[k], eb[k]), (what, k, np.argwhere(ea[k] != eb[k])[:5].tolist())
    return ea
