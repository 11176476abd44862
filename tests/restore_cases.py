"""What the tests of the indexed restore (tests/test_restore_indexed.py) share: the shapes, the index patterns, and the expectation — an
OracleVecEnv whose saved state is rearranged with the same index in plain numpy.  Nothing here touches an engine."""
import numpy as np

from models import EpisodeModel

P_ACT = [.05, .7, .1, .1, .05]
TINY = dict(shelf_columns=3, column_height=8, shelf_rows=1, n_agents=2)
# name -> (envs, constructor keywords): the smallest shapes at which the gather can go wrong
SHAPES = {
    "tiny-7": (7, TINY),                                                                    # 110-byte shadow rows, one ragged workgroup
    "tiny-300": (300, TINY),                                                                # several workgroups, the last one ragged
    "wide-4x16": (9, dict(shelf_columns=5, column_height=1, shelf_rows=1, n_agents=3)),     # 12-byte record rows, W > H
    "29x28-10ag": (5, dict(shelf_columns=9, column_height=8, shelf_rows=3, n_agents=10)),   # > 255 shelves: 2-byte shadow cells
    "msg": (6, dict(TINY, msg_bits=2)),                                                     # the message piece
    "70ag": (5, dict(TINY, n_agents=70)),                                                   # rows past 64 agents
}
PATTERNS = ("identity", "none", "reversal", "one-slot", "random")


def index_pattern(kind, B):
    """int32 (B,): env e takes slot index[e]; -1 keeps env e"""
    if kind == "identity":
        return np.arange(B, dtype=np.int32)
    if kind == "none":
        return np.full(B, -1, np.int32)
    if kind == "reversal":
        return np.arange(B, dtype=np.int32)[::-1].copy()
    if kind == "one-slot":
        return np.full(B, B // 2, np.int32)
    assert kind == "random"
    rng = np.random.default_rng(17)
    idx = rng.integers(0, B, size=B).astype(np.int32)
    idx[1] = idx[0]                                              # at least one slot taken twice
    idx[2::3] = -1                                               # a third untouched, between restored ones
    return idx


class Saved:
    """the whole state of an OracleVecEnv (its FIELDS arrays, agent_msg, the pending NEXT_STEP resets, the two event counters) and of the
    episode model beside it, copied"""

    def __init__(self, orc, episodes=None):
        self.f = {k: getattr(orc, k).copy() for k in orc.FIELDS + ("agent_msg", "stat_deliveries", "stat_failed_moves")}
        self.f["_prev_done"] = getattr(orc, "_prev_done", np.zeros(orc.B, np.uint8)).copy()
        self.ep = None if episodes is None else ({k: v.copy() for k, v in episodes.v.items()}, episodes.pending.copy())


def rearrange(orc, saved, index, keep_rng=False, episodes=None):
    """the oracle after "env e <- saved slot index[e]; -1 keeps env e", in numpy"""
    index = np.asarray(index)
    hit = index >= 0
    src = index[hit]
    if not hasattr(orc, "_prev_done"):
        orc._prev_done = np.zeros(orc.B, np.uint8)
    for k, v in saved.f.items():
        if k == "rng" and keep_rng:
            continue
        getattr(orc, k)[hit] = v[src]
    if episodes is not None:
        vals, pending = saved.ep
        for k in episodes.v:
            episodes.v[k][hit] = vals[k][src]
        episodes.pending[hit] = pending[src]
    return hit


def play(env, orc, rng, steps, mode="next_step", episodes=None):
    """`steps` random steps of both; the env may be None (the oracle alone)"""
    N, M = orc.N, orc.M
    for _ in range(steps):
        a = rng.choice(5, size=(orc.B, N), p=P_ACT).astype(np.int32)
        if M:
            a = np.concatenate([a[..., None], rng.integers(0, 2, size=(orc.B, N, M)).astype(np.int32)], axis=-1)
        if env is not None:
            env.step(a)
        _, rew, done = orc.step_autoreset(a, mode)
        if episodes is not None:
            episodes.step(rew, done)


def episode_model(orc, mode="next_step"):
    return EpisodeModel(orc.B, orc.N, mode)
