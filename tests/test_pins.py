"""tests/pins.py's own proof: every field check_state / check_rewards can compare goes red.

Every constructed pin replays its fixture through pins.check_state, so a field that check silently skipped would pass on every
backend.  Here, on the oracle alone: 8 scenarios of handling/tiny-2ag (the five agent fields, shelves, queue, both counters, the
generator words, rewards, done) over the first 4 of their steps, and 8 of observations/tiny-3ag-msg1 (`agent_msg`) over the 2 steps that
fixture records.  Unperturbed the replay passes; with ONE element of ONE compared field changed behind ONE step it raises, and the
message names the scenario and that step.
"""
import os

import numpy as np
import pytest

import handling_scenarios as hs
import lockstep
import pins
import rware_amd
from rware_oracle import OracleVecEnv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMPARED = pins.STATE_FIELDS + ("rewards", "done")


def name_of(task, z, k, t):
    return f"{task}, scenario {k} ({z['variant'][k]}), step {t}"


def handling():
    """(task, fixture under TWO_STAGE with the limits set, constructor arguments, steps, fields recorded)"""
    c = hs.CONFIGS.index((hs.TWO_STAGE, True))
    z = pins.load_npz(os.path.join(GOLDEN, "handling"), "tiny-2ag")
    kw = dict(lockstep.oracle_kwargs(z["meta"]["env_id"], **z["meta"]["overrides"]), **hs.config_shape({}, c))
    return "tiny-2ag", hs.config_view(z, c), kw, 4, tuple(f for f in pins.STATE_FIELDS if f != "agent_msg")


def cleared_flags(z):
    z["agent_delivered"] = np.zeros_like(z["agent_x"])


def observations():
    """(task, fixture with the flags its generator clears, constructor arguments, steps, fields recorded)"""
    z = pins.load_npz(os.path.join(GOLDEN, "observations"), "tiny-3ag-msg1", prepare=cleared_flags)
    kw = dict(rware_amd.env_kwargs(z["meta"]["env_id"]), **z["meta"]["kwargs"])
    kw["reward_type"] = rware_amd.enums.enum_value(kw["reward_type"])
    assert z["meta"]["M"] == 1 and (z["reward_type"][:8] == kw["reward_type"]).all()
    return "tiny-3ag-msg1", z, kw, z["meta"]["steps"], pins.AGENT_FIELDS + ("agent_msg", "shelf_xy", "queue", "rng")


def replay(pin, corrupt=None):
    """The first 8 scenarios on the oracle, every recorded field of every step through pins.check_state.
    `corrupt` = (field, step): one element of that field is changed behind that step, and nothing else."""
    task, z, kw, steps, fields = pin()
    idx = np.arange(8)
    orc = OracleVecEnv(len(idx), **kw)
    pins.inject(orc, z, idx)
    for t in range(steps):
        rew, done = orc.step(z["actions"][idx, t].astype(np.int32))
        got = dict(orc.get_state(), shelf_xy=orc.shelf_xy(), rewards=rew, done=done)
        if corrupt is not None and corrupt[1] == t:
            a = np.array(got[corrupt[0]])
            a.flat[a.size // 2] = 1 - a.flat[a.size // 2] if corrupt[0] == "done" else a.flat[a.size // 2] + 1
            got[corrupt[0]] = a
        pins.check_state(task, z, idx, t, got, got["shelf_xy"], got["rewards"], got["done"], "oracle: ", fields=fields, name_of=name_of)


@pytest.mark.parametrize("pin", [handling, observations])
def test_the_uncorrupted_replay_passes(pin):
    replay(pin)


def test_the_two_pins_reach_every_field_the_checks_compare():
    assert set(handling()[4]) | set(observations()[4]) == set(pins.STATE_FIELDS)


@pytest.mark.parametrize("field", COMPARED)
def test_one_corrupted_element_fails_the_shared_check(field):
    pin = observations if field == "agent_msg" else handling
    task, _, _, steps, fields = pin()
    assert field in fields + ("rewards", "done")
    for step in (0, steps - 1):
        with pytest.raises(AssertionError) as err:
            replay(pin, corrupt=(field, step))
        msg = str(err.value)
        assert msg.startswith(f"oracle: {task}, scenario ") and f"step {step}" in msg, msg
        if field in pins.AGENT_FIELDS + ("agent_msg", "rewards"):
            assert "agent " in msg, msg
        elif field != "done":
            assert field.replace("shelf_xy", "shelf ") in msg, msg
