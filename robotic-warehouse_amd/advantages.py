"""GAE(lambda) advantages and returns from rollout tapes, on the host: `gae` is the definition of include/rware_hip_advantages.h (rw_gae,
WarehouseVecEnv.gae_device) written in float32 numpy operations, one separately rounded operation after the other in the same order, so
its results equal the device's bit for bit.  For output="numpy" users, and as executable documentation of what the kernel computes.

Four facts about the engine's tapes that the computation builds on:
  - NEXT_STEP autoreset (the default): the step after an episode end is a reset step — action ignored, reward 0, no flags — and the
    observation it acted on is the terminal one.  So values[t + 1] is already V(final obs), the bootstrap of a truncated end, and the
    reset step itself is no transition: its advantage is 0 and `valid` is False there.
  - SAME_STEP (and DISABLED with reset(mask=terminated) inside the loop): obs[t + 1] is the new episode's first observation; a truncated
    end bootstraps from V(final_obs), which the caller supplies as `final_values`, or from 0.
  - `terminated` ends without a bootstrap, `truncated` (time_limit_truncates=True) ends with one.
  - under NEXT_STEP, whether step 0 of a tape is a reset step depends on the last row of the tape before it: `prev_ended`."""
from __future__ import annotations

import numpy as np


def gae_shapes(rewards_shape, values_shape, last_values_shape):
    """The shapes of gae() / gae_device(), checked -> (T, B, N, K, shape of advantages and returns).  `values` is (T+1, B[, K]) without
    `last_values` (row T is the bootstrap), else (T, B[, K]) with `last_values` (B[, K])."""
    if len(rewards_shape) != 3:
        raise ValueError(f"`rewards` must be (T, B, N), got {tuple(rewards_shape)}")
    T, B, N = (int(v) for v in rewards_shape)
    rows = T + 1 if last_values_shape is None else T
    if len(values_shape) not in (2, 3) or tuple(values_shape[:2]) != (rows, B):
        raise ValueError(f"`values` must be ({rows}, {B}) or ({rows}, {B}, K) " + ("without" if last_values_shape is None else "with") +
                         f" `last_values`, got {tuple(values_shape)}")
    K = int(values_shape[2]) if len(values_shape) == 3 else 1
    if K != 1 and K != N:
        raise ValueError(f"`values` has {K} heads per env: neither 1 nor the {N} agents of `rewards`")
    if last_values_shape is not None and tuple(last_values_shape) != tuple(values_shape[1:]):
        raise ValueError(f"`last_values` must be {tuple(values_shape[1:])}, got {tuple(last_values_shape)}")
    return T, B, N, K, (T,) + tuple(int(v) for v in values_shape[1:])


def _flags(x, shape, name):
    a = np.asarray(x)
    if a.dtype not in (np.dtype(bool), np.dtype(np.uint8)) or a.shape != shape:
        raise ValueError(f"`{name}` must be bool or uint8 {shape}, got {a.dtype} {a.shape}")
    return a != 0


def gae(rewards, values, terminated, truncated=None, last_values=None, final_values=None, prev_ended=None, gamma=0.99, lam=0.95,
        team_reward=None, next_step=None, out=None):
    """-> (advantages, returns, valid): float32 arrays of the shape of values[:T] and a bool (T, B) mask, False on reset steps.

    `rewards` float32 (T, B, N); `values` float32 (T+1, B[, K]) with row T the bootstrap, or (T, B[, K]) with `last_values` (B[, K]);
    K == N a per-agent critic, K == 1 (or no K axis) one value per env.  `terminated`, `truncated` (None: all False): bool or uint8
    (T, B).  `next_step` (None: True, the engine's default autoreset mode): the tape was written under NEXT_STEP autoreset — then
    `prev_ended` (B,), the last row's terminated | truncated of the tape before this one, says whether step 0 is a reset step (None: no),
    and `final_values` is ignored; else a truncated end bootstraps from `final_values` (the shape of values[:T]; None: from 0), which is
    read only where truncated and not terminated, and `prev_ended` is ignored.  `team_reward` (None: K == 1 and N > 1): every head sees
    the env's rewards summed left to right.  `out`: an optional triple of arrays to write into.
    Per column, backwards in time, in float32 with g = gamma and gl = float32(gamma * lam):
        boot  = 0 if terminated, else V(final obs) if truncated — values[t + 1] under NEXT_STEP —, else values[t + 1]
        delta = (r + g * boot) - values[t]
        adv   = delta if the step ended an episode, else delta + gl * adv[t + 1];  0 on a reset step, whatever its flags
        returns = adv + values[t]
    ValueError for wrong shapes or dtypes and for gamma or lam outside [0, 1]."""
    f32 = np.float32
    r, vals = np.asarray(rewards), np.asarray(values)
    last = None if last_values is None else np.asarray(last_values)
    if r.dtype != f32 or vals.dtype != f32 or (last is not None and last.dtype != f32):
        raise ValueError("`rewards`, `values` and `last_values` must be float32")
    T, B, N, K, shape = gae_shapes(r.shape, vals.shape, None if last is None else last.shape)
    if not (0.0 <= float(gamma) <= 1.0 and 0.0 <= float(lam) <= 1.0):
        raise ValueError(f"gamma ({gamma}) and lam ({lam}) must lie in [0, 1]")
    team = (K == 1 and N > 1) if team_reward is None else bool(team_reward)
    if K == 1 and N > 1 and not team:
        raise ValueError("one value head over several agents needs team_reward")
    ns = True if next_step is None else bool(next_step)
    term = _flags(terminated, (T, B), "terminated")
    trunc = np.zeros((T, B), bool) if truncated is None else _flags(truncated, (T, B), "truncated")
    prev = np.zeros(B, bool) if prev_ended is None or not ns else _flags(prev_ended, (B,), "prev_ended")
    fv = None
    if final_values is not None and not ns:
        fv = np.asarray(final_values)
        if fv.dtype != f32 or fv.shape != shape:
            raise ValueError(f"`final_values` must be float32 {shape}, got {fv.dtype} {fv.shape}")
        fv = fv.reshape(T, B, K)
    if last is None:
        vals, last = vals[:T], vals[T]
    vals, last = vals.reshape(T, B, K), last.reshape(B, K)
    if team:
        acc = r[:, :, 0] if N else np.zeros((T, B), f32)
        for i in range(1, N):
            acc = acc + r[:, :, i]
        r = np.broadcast_to(acc[:, :, None], (T, B, K))
    adv, ret, valid = np.empty((T, B, K), f32), np.empty((T, B, K), f32), np.empty((T, B), bool)
    g = f32(gamma)
    gl = f32(g * f32(lam))
    carry, next_v, zero = np.zeros((B, K), f32), last.astype(f32, copy=True), np.zeros((B, K), f32)
    ended = term | trunc
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            v = vals[t]
            te, tr = term[t][:, None], trunc[t][:, None]
            reset = (ended[t - 1] if t > 0 else prev)[:, None] if ns else np.zeros((B, 1), bool)
            boot = np.where(te, zero, np.where(tr, next_v if ns else (zero if fv is None else fv[t]), next_v))
            delta = (r[t] + g * boot) - v
            a = np.where(te | tr, delta, delta + gl * carry)
            a = np.where(reset, zero, a)
            adv[t], ret[t], valid[t] = a, a + v, ~reset[:, 0]
            carry, next_v = a, v
    adv, ret = adv.reshape(shape), ret.reshape(shape)
    if out is not None:
        for o, x, name in zip(out, (adv, ret, valid), ("advantages", "returns", "valid")):
            if not isinstance(o, np.ndarray) or o.shape != x.shape or o.dtype != x.dtype:
                raise ValueError(f"`out`: {name} must be a {x.dtype} array of shape {x.shape}")
            o[...] = x
        return tuple(out)
    return adv, ret, valid
