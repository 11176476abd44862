"""The one env-beside-oracle loop of the suite: a WarehouseVecEnv (emulated or on the device) and an OracleVecEnv reset and stepped on
the same actions, every field compared.  A failure names the field, the step and the first differing indices — the same message
on the emulation and on the device."""
import enum
from collections import namedtuple

import numpy as np

import rware_amd

Run = namedtuple("Run", "steps episodes finals")   # steps run, episodes ended (done flags seen), terminal observations compared


def oracle_kwargs(env_id=None, **extra):
    """The registered id's constructor arguments with `extra` applied and enum values reduced to ints: ONE dict that constructs both
    the env and the oracle."""
    kw = rware_amd.env_kwargs(env_id) if env_id else {}
    kw.update(extra)
    return {k: v.value if isinstance(v, enum.Enum) else v for k, v in kw.items()}


def attempt(f):
    """(result, raised_IndexError) — the transposed image layers raise where the reference does."""
    try:
        return f(), False
    except IndexError:
        return None, True


def _same(got, want, what, t):
    g, w = np.asarray(got), np.asarray(want)
    if g.dtype == np.bool_ or w.dtype == np.bool_:    # (flags: the oracle's are uint8 0/1)
        g, w = g.astype(bool), w.astype(bool)
    if g.shape != w.shape:
        raise AssertionError(f"{what} at step {t}: shape {g.shape} != {w.shape}")
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)[:5]
        raise AssertionError(f"{what} differs at step {t}: first idx {bad.tolist()}")


def same_obs(got, want, what="obs", t=None, rows=None):
    """FLATTENED / IMAGE arrays, or the env's IMAGE_DICT {"image", "features"} against the oracle's (image, features); `rows`: a mask."""
    pick = (lambda a: a) if rows is None else (lambda a: np.asarray(a)[rows])
    if isinstance(got, dict):
        assert isinstance(want, tuple), f"{what} at step {t}: the env gave a dict, the oracle {type(want).__name__}"
        _same(pick(got["image"]), pick(want[0]), f"{what} image", t)
        _same(pick(got["features"]), pick(want[1]), f"{what} features", t)
    else:
        _same(pick(got), pick(want), what, t)


def same_state(got, want, t=None):
    """Every field of get_state()."""
    for k in want:
        _same(got[k], want[k], f"state field {k}", t)


def lockstep(env, orc, actions, mode="next_step", *, seed, steps=None, t0=0, state_every=None, final_obs=None, on_step=None, skip=()):
    """Resets both (`seed=None`: continues a pair that is already in step) and steps them on `actions` — a (T, B, N[, 1+M]) array, or
    a callable t -> actions with `steps` — in autoreset mode `mode`.  Compared: the reset observation; per step the observation,
    the rewards and `terminated`, `truncated` all-False; under same_step (`final_obs` None: by the mode) the ("final_obs" in info)
    == done.any() rule, info["_final_obs"] and the masked info["final_obs"]; every `state_every` steps and after the last one every
    field of get_state().  `on_step(t, obs, rew, term, info)` runs after a step's comparisons; `skip` names comparisons
    ("terminated", "state") to leave out.  Step numbers in messages start at `t0`."""
    if seed is not None:
        same_obs(env.reset(seed=seed)[0], orc.reset(seed=seed), "reset obs", "reset")
    T = len(actions) if steps is None else steps
    final_obs = (mode == "same_step") if final_obs is None else final_obs
    episodes = finals = 0
    for i in range(T):
        t = t0 + i
        a = actions(t) if callable(actions) else actions[i]
        obs, rew, term, trunc, info = env.step(a)
        o2, r2, d2 = orc.step_autoreset(a, mode)
        _same(rew, r2, "rewards", t)
        if "terminated" not in skip:
            _same(term, d2.astype(bool), "terminated", t)
        assert not np.asarray(trunc).any(), f"truncated set at step {t}"
        same_obs(obs, o2, "obs", t)
        episodes += int(d2.sum())
        if final_obs:
            assert ("final_obs" in info) == bool(d2.any()), f"final_obs in info == done.any() broken at step {t}"
            if d2.any():
                m = orc.final_mask
                _same(info["_final_obs"], m, "_final_obs", t)
                same_obs(info["final_obs"], orc.final_obs, "final_obs", t, rows=m)
                finals += int(m.sum())
        else:
            assert "final_obs" not in info, f"final_obs in info at step {t} without same_step autoreset"
        if "state" not in skip and ((state_every and i % state_every == 0) or i == T - 1):
            same_state(env.get_state(), orc.get_state(), t)
        if on_step is not None:
            on_step(t, obs, rew, term, info)
    return Run(T, episodes, finals)


def check_rollout(env, orc, actions, mode="next_step", *, t0=0, want_obs=True, n_obs=None, state=True):
    """env.rollout(actions) against the oracle stepped over the same tape: the observation tape (IMAGE_DICT: the image tape; its first
    `n_obs` steps when given), rewards and `terminated` of every step, then every field of get_state()."""
    tape, rew, term = env.rollout(actions) if want_obs else env.rollout(actions, want_obs=False)
    for k in range(len(actions)):
        o2, r2, d2 = orc.step_autoreset(actions[k], mode)
        _same(rew[k], r2, "rollout rewards", t0 + k)
        _same(term[k], d2.astype(bool), "rollout terminated", t0 + k)
        if want_obs and (n_obs is None or k < n_obs):
            _same(tape[k], o2[0] if isinstance(o2, tuple) else o2, "rollout obs", t0 + k)
    if state:
        same_state(env.get_state(), orc.get_state(), t0 + len(actions) - 1)
    return Run(len(actions), int(np.asarray(term).sum()), 0)
