"""The lockstep harness (tests/lockstep.py) checked on its own, without a GPU or the emulation library: an OracleVecEnv behind
WarehouseVecEnv's reset / step / rollout / get_state surface runs beside a second oracle.  Unperturbed it passes in all three
autoreset modes; with ONE element of ONE compared field corrupted at ONE step — nothing else about the adapter changes — the
harness must raise and name the field and the step."""
import numpy as np
import pytest

from lockstep import check_rollout, lockstep, oracle_kwargs
from rware_oracle import OracleVecEnv

B, T = 4, 30
MODES = ["next_step", "same_step", "disabled"]


class OracleAsEnv:
    """An oracle with the env's call surface; `corrupt=(field, step)` changes one element of that field at that step (`step` counts
    step() calls, or the rows of a rollout tape; "reset" for the reset observation)."""

    def __init__(self, mode, corrupt=(None, None), **kw):
        self.orc, self.mode, self.corrupt, self.t = OracleVecEnv(B, **kw), mode, corrupt, 0

    def _hit(self, field, t):
        return self.corrupt == (field, t)

    @staticmethod
    def _flip(a):
        a = np.array(a)
        a.flat[a.size // 2] = 1 - a.flat[a.size // 2]
        return a

    def _obs(self, o, field, t, part="image"):
        if isinstance(o, tuple):
            o = {"image": o[0], "features": o[1]}
            if self._hit("features", t):
                o["features"] = self._flip(o["features"])
            if self._hit(field, t):
                o[part] = self._flip(o[part])
        elif self._hit(field, t):
            o = self._flip(o)
        return o

    def reset(self, seed=None):
        return self._obs(self.orc.reset(seed=seed), "reset obs", "reset"), {}

    def step(self, a):
        t, self.t = self.t, self.t + 1
        o, r, d = self.orc.step_autoreset(a, self.mode)
        term = d.astype(bool)
        info = {}
        if self.mode == "same_step" and d.any():
            info = {"final_obs": self.orc.final_obs, "_final_obs": self.orc.final_mask.copy()}
            if isinstance(info["final_obs"], tuple):
                info["final_obs"] = {"image": info["final_obs"][0], "features": info["final_obs"][1]}
            if self._hit("_final_obs", t):
                info["_final_obs"] = ~info["_final_obs"]
            if self._hit("final_obs", t):            # one element of a row that ended: the rows outside the mask are not compared
                f = info["final_obs"]["image"] if isinstance(info["final_obs"], dict) else info["final_obs"]
                f = np.array(f)
                row = f[int(np.argmax(self.orc.final_mask))]
                row.flat[0] = 1 - row.flat[0]
                info["final_obs"] = dict(info["final_obs"], image=f) if isinstance(info["final_obs"], dict) else f
        if self._hit("rewards", t):
            r = self._flip(r)
        if self._hit("terminated", t):
            term = self._flip(term.astype(np.uint8)).astype(bool)
        return self._obs(o, "obs", t), r, term, np.zeros(B, bool), info

    def rollout(self, acts, want_obs=True):
        outs = [self.orc.step_autoreset(a, self.mode) for a in acts]
        tape = np.stack([o[0][0] if isinstance(o[0], tuple) else o[0] for o in outs])
        if self.corrupt[0] == "rollout obs":
            tape[self.corrupt[1]] = self._flip(tape[self.corrupt[1]])
        return (tape if want_obs else None), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs]).astype(bool)

    def get_state(self):
        st = self.orc.get_state()
        if self.corrupt[0] == "agent_dir" and self.t == self.corrupt[1] + 1:
            st["agent_dir"] = self._flip(st["agent_dir"])
        return st


def _pair(mode, corrupt=(None, None), **extra):
    kw = oracle_kwargs("rware-tiny-2ag-v1", max_steps=10, **extra)     # (episodes end within the 30 steps)
    return OracleAsEnv(mode, corrupt, **kw), OracleVecEnv(B, **kw)


def _tape(seed=0):
    return np.random.default_rng(seed).choice(5, size=(T, B, 2), p=[.1, .55, .1, .1, .15]).astype(np.int32)


def test_oracle_kwargs_reduces_enums_and_applies_extras():
    kw = oracle_kwargs("rware-tiny-2ag-v1", max_steps=10, observation_type=3)
    assert kw["max_steps"] == 10 and kw["observation_type"] == 3 and kw["n_agents"] == 2
    assert all(type(v) in (int, bool, float, str, list, tuple, type(None)) for v in kw.values()), kw


@pytest.mark.parametrize("obs_type", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_an_oracle_behind_the_env_surface_passes(mode, obs_type):
    env, orc = _pair(mode, observation_type=obs_type, sensor_range=1)
    acts = _tape()
    seen = []
    run = lockstep(env, orc, acts, mode, seed=5, state_every=7, on_step=lambda t, o, r, d, info: seen.append(t))
    assert run.steps == T and seen == list(range(T)) and run.episodes >= 2 * B
    assert run.finals == (run.episodes if mode == "same_step" else 0)
    rng = np.random.default_rng(1)     # a callable, continuing the same pair without a reset
    run = lockstep(env, orc, lambda t: rng.integers(0, 5, size=(B, 2), dtype=np.int32), mode, seed=None, steps=5, t0=T)
    assert run.steps == 5
    assert check_rollout(env, orc, _tape(2), mode, t0=T + 5).steps == T


@pytest.mark.parametrize("field,step,obs_type,mode", [
    ("reset obs", "reset", 1, "next_step"),
    ("obs", 17, 1, "next_step"),
    ("obs", 0, 2, "disabled"),
    ("obs", 29, 3, "same_step"),            # the image of an IMAGE_DICT observation
    ("features", 13, 3, "next_step"),
    ("rewards", 21, 1, "same_step"),
    ("terminated", 4, 1, "next_step"),
    ("agent_dir", 14, 1, "next_step"),      # one get_state() field, at a periodic state check
    ("agent_dir", 29, 1, "next_step"),      # ... and at the one after the last step
    ("_final_obs", 9, 1, "same_step"),      # (max_steps=10: every env ends its first episode at step 9)
    ("final_obs", 9, 1, "same_step"),
    ("final_obs", 19, 3, "same_step"),
])
def test_one_corrupted_element_is_caught_and_named(field, step, obs_type, mode):
    env, orc = _pair(mode, (field, step), observation_type=obs_type)
    with pytest.raises(AssertionError) as ei:
        lockstep(env, orc, _tape(), mode, seed=5, state_every=7)
    msg = str(ei.value)
    assert field in msg and f"step {step}" in msg and "first idx" in msg, msg
    assert env.t == (0 if step == "reset" else step + 1)     # raised AT that step, not later


@pytest.mark.parametrize("obs_type,mode", [(1, "next_step"), (3, "same_step")])
def test_one_corrupted_element_of_the_rollout_tape_is_caught_and_named(obs_type, mode):
    env, orc = _pair(mode, ("rollout obs", 11), observation_type=obs_type)
    lockstep(env, orc, _tape(), mode, seed=5)                # (the stepwise part is untouched: it passes)
    with pytest.raises(AssertionError) as ei:
        check_rollout(env, orc, _tape(3), mode, t0=T)
    assert "rollout obs" in str(ei.value) and f"step {T + 11}" in str(ei.value), str(ei.value)


def test_truncated_and_stray_final_obs_are_refused():
    env, orc = _pair("next_step")
    env.step = lambda a, step=env.step: step(a)[:3] + (np.ones(B, bool), {})
    with pytest.raises(AssertionError, match="truncated set at step 0"):
        lockstep(env, orc, _tape(), seed=5)
    env, orc = _pair("next_step")
    env.step = lambda a, step=env.step: step(a)[:4] + ({"final_obs": None},)
    with pytest.raises(AssertionError, match="final_obs in info at step 0"):
        lockstep(env, orc, _tape(), seed=5)
    env, orc = _pair("same_step")
    env.step = lambda a, step=env.step: step(a)[:4] + ({},)     # the terminal observation withheld
    with pytest.raises(AssertionError, match="final_obs in info == done.any.. broken at step 9"):
        lockstep(env, orc, _tape(), "same_step", seed=5)
