"""rw_gae: GAE(lambda) advantages and returns from a rollout's reward, flag and value tapes in one launch — the kernel
(csrc/rware_advantages.h), Engine.gae, WarehouseVecEnv.gae_device and the host function rware_amd.gae.

  - CPU suite: the product sources on host threads (tests/emu; a device pointer is a host pointer there).
  - GPU suite (-m gpu): the same checks on the gfx950 library, then the torch surface and a captured call.
Expectations never come from the code under test: `model` below is the definition of include/rware_hip_advantages.h in float32 numpy
operations, one rounded operation at a time, and `episodes_f64` an independent float64 computation that first cuts every column into
episodes and then runs textbook GAE inside each.  Device results are compared with the model by exact equality of bit patterns; outputs
lie in poisoned memory between two guards (device_backends.alloc)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import lockstep
from device_backends import BACKENDS, GUARD, POISON

import rware_amd
from rware_amd import _capi

OK, INVALID = _capi.RW_OK, _capi.RW_ERR_INVALID_ARG
f32 = np.float32
# (T, B, N, K, team): the smallest shapes at which the chunking can go wrong
SHAPES = {
    "one": (1, 1, 1, 1, False),
    "6-columns": (2, 3, 2, 2, False),          # no whole 16-byte group of columns
    "12-columns": (9, 4, 3, 3, False),         # 16-byte groups straddle envs (chunks of four steps there); T = 9: a whole chunk and a tail
    "team-1-head": (9, 5, 3, 1, True),
    "team-3-heads": (9, 4, 3, 3, True),
    "65-agents": (5, 2, 65, 65, False),
    "team-65-agents": (5, 2, 65, 1, True),     # the sum crosses agent 64
    "280-columns": (3, 70, 4, 4, False),       # 70 threads of 4 columns, 280 of one: more than a 64-thread workgroup, by no multiple
    "20-steps": (20, 5, 4, 4, False),          # K % 4 == 0: the one-env-a-lane build, five chunks of four steps; one column a lane: two of eight and a tail
    "17-steps-team": (17, 3, 8, 8, True),      # the one-column build with the sum: two chunks of eight and one step
}
GAMMAS = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.5), (0.9, 0.0)]


# ------------------------------------------------------------------------------------------------ the two references
def team_sum(rew):
    acc = rew[:, :, 0]
    for i in range(1, rew.shape[2]):
        acc = acc + rew[:, :, i]
    return acc


def model(rew, val, last, term, trunc, fv, prev, gamma, lam, ns, team):
    """The definition, in float32: rew (T, B, N), val (T, B, K), last (B, K) float32; term, trunc (None: zeros) (T, B), prev (None: zeros)
    (B,) uint8, non-zero = set; fv (T, B, K) or None.  -> advantages, returns (T, B, K) float32, valid (T, B) uint8"""
    T, B, K = val.shape
    assert rew.dtype == val.dtype == last.dtype == f32
    g = f32(gamma)
    gl = g * f32(lam)
    assert type(gl) is f32
    r = np.repeat(team_sum(rew)[:, :, None], K, axis=2) if team else rew
    te = term != 0
    tr = np.zeros((T, B), bool) if trunc is None else trunc != 0
    pe = np.zeros(B, bool) if prev is None else prev != 0
    adv, ret, valid = np.zeros((T, B, K), f32), np.zeros((T, B, K), f32), np.zeros((T, B), np.uint8)
    carry, next_v = np.zeros((B, K), f32), last.copy()
    with np.errstate(all="ignore"):
        for t in reversed(range(T)):
            is_reset = np.zeros(B, bool) if not ns else (te[t - 1] | tr[t - 1]) if t > 0 else pe
            on_trunc = next_v if ns else fv[t] if fv is not None else np.zeros((B, K), f32)
            boot = np.where(te[t][:, None], f32(0), np.where(tr[t][:, None], on_trunc, next_v))
            p = g * boot
            s = r[t] + p
            delta = s - val[t]
            q = gl * carry
            a = np.where((te[t] | tr[t])[:, None], delta, delta + q)
            a = np.where(is_reset[:, None], f32(0), a)
            assert a.dtype == f32
            adv[t], ret[t], valid[t] = a, a + val[t], ~is_reset
            carry, next_v = a, val[t]
    return adv, ret, valid


def episodes_f64(rew, val, last, term, trunc, fv, prev, gamma, lam, ns, team):
    """Independent of `model`: every column is cut into episodes first — under NEXT_STEP the step after an end is a reset step and belongs
    to none —, each episode gets the bootstrap the engine's autoreset mode implies, and textbook GAE runs inside it in float64.
    (gamma and gamma * lambda are the float32 parameters of the definition, taken to float64; a team reward is the definition's float32
    sum: the bound below counts the five roundings of a step, not those.)  -> advantages (T, B, K) float64, valid (T, B) bool"""
    T, B, K = val.shape
    g = float(f32(gamma))
    gl = float(f32(gamma) * f32(lam))
    r = (np.repeat(team_sum(rew)[:, :, None], K, axis=2) if team else rew).astype(np.float64)
    v64 = val.astype(np.float64)
    adv, valid = np.zeros((T, B, K)), np.ones((T, B), bool)
    for b in range(B):
        ended = [(term[t, b] != 0) or (trunc is not None and trunc[t, b] != 0) for t in range(T)]
        after_end = bool(prev is not None and prev[b] != 0) if ns else False
        episodes, cur = [], []
        for t in range(T):
            if ns and after_end:                  # a reset step: no transition (whatever flags a constructed tape gives it)
                valid[t, b] = False
                after_end = ended[t]
                continue
            cur.append(t)
            after_end = ended[t]
            if ended[t]:
                episodes.append(cur)
                cur = []
        if cur:
            episodes.append(cur)
        for ep in episodes:
            end = ep[-1]
            for k in range(K):
                after = v64[end + 1, b, k] if end + 1 < T else float(last[b, k])     # V of the observation the next step acts on
                if term[end, b] != 0:
                    boot = 0.0
                elif trunc is not None and trunc[end, b] != 0:
                    boot = after if ns else float(fv[end, b, k]) if fv is not None else 0.0   # NEXT_STEP: that observation is the final one
                else:
                    boot = after                                                             # the tape ends inside the episode
                a_next, v_next = 0.0, boot
                for t in reversed(ep):
                    a_next = r[t, b, k] + g * v_next - v64[t, b, k] + gl * a_next
                    adv[t, b, k] = a_next
                    v_next = v64[t, b, k]
    return adv, valid


def bound(T, adv64, val, rew_seen):
    """five roundings a step, each at most 2^-24 of an intermediate bounded by A; they propagate with a factor gamma * lambda <= 1"""
    A = max(1.0, float(np.abs(adv64).max(initial=0)) + float(np.abs(val).max(initial=0)) + float(np.abs(rew_seen).max(initial=0)))
    return 5 * T * 2.0 ** -24 * A


def random_tape(rng, T, B, N, K, rate=0.2):
    """everything rw_gae can read, random: flags set at `rate` each (a set byte is any non-zero value)"""
    flag = lambda shape, p: (rng.random(shape) < p) * rng.choice([1, 1, 2, 255], size=shape).astype(np.uint8)
    return dict(rew=rng.normal(size=(T, B, N)).astype(f32), val=rng.normal(size=(T, B, K)).astype(f32) * f32(3),
                last=rng.normal(size=(B, K)).astype(f32), fv=rng.normal(size=(T, B, K)).astype(f32),
                term=flag((T, B), rate).astype(np.uint8), trunc=flag((T, B), rate).astype(np.uint8), prev=flag((B,), 0.5).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ device arrays
class Output:
    """a poisoned device array with a guard on either side of `count` elements of `size` bytes, the payload `offset_elems` elements
    behind a 16-byte boundary"""

    def __init__(self, be, count, size, offset_elems=0):
        self.lo, self.n = GUARD + offset_elems * size, count * size
        self.keep, base, self.read = be.alloc(self.lo + self.n + GUARD)
        assert base % 16 == 0
        self.ptr = base + self.lo

    def check(self, want, what):
        raw = self.read()
        assert (raw[:self.lo] == POISON).all() and (raw[self.lo + self.n:] == POISON).all(), f"{what}: a guard was written"
        bits = np.uint32 if want.dtype == f32 else np.uint8
        got, want = raw[self.lo:self.lo + self.n].view(bits).reshape(want.shape), want.view(bits)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{what}: {len(bad)} of {want.size} differ, first at {bad[:5].tolist()}: got "
                                 f"{[hex(got[tuple(b)]) for b in bad[:5]]}, want {[hex(want[tuple(b)]) for b in bad[:5]]}")

    def untouched(self, what):
        assert (self.read() == POISON).all(), f"{what}: something was written"


def place(be, a, offset_elems=0):
    """-> the device pointer of a copy of `a` that starts `offset_elems` elements behind a 16-byte boundary"""
    flat = np.ascontiguousarray(a).reshape(-1)
    size = flat.itemsize
    buf = np.zeros(flat.size + 16 // size + offset_elems + 1, flat.dtype)
    at = offset_elems if be.gpu else ((-buf.ctypes.data) % 16) // size + offset_elems
    buf[at:at + flat.size] = flat
    base = be.ptr(buf)
    assert be.gpu or base == buf.ctypes.data
    p = base + at * size
    assert p % 16 == (offset_elems * size) % 16
    return p


def make_engine(be):
    """the engine gives rw_gae its device and its stream only: any will do"""
    env = rware_amd.WarehouseVecEnv(2, library=be.library(), **dict(lockstep.oracle_kwargs("rware-tiny-2ag-v1"), **be.kw))
    return env, env.engines[0]


def run_op(be, eng, ptrs, shape, gamma, lam, ns, team, use, off=0):
    """one rw_gae call into fresh poisoned outputs -> (advantages, returns or None, valid or None) Output objects; `use`: which of the
    optional arrays are handed over (the others NULL)"""
    T, B, N, K = shape
    adv = Output(be, T * B * K, 4, off)
    ret = Output(be, T * B * K, 4, off) if use["returns"] else None
    valid = Output(be, T * B, 1, off) if use["valid"] else None
    eng.gae(ptrs["rew"], ptrs["val"], ptrs["last"], ptrs["term"], adv.ptr, T, B, N, K,
            truncated_ptr=ptrs["trunc"] if use["trunc"] else 0, final_values_ptr=ptrs["fv"] if use["fv"] else 0,
            prev_ended_ptr=ptrs["prev"] if use["prev"] else 0, returns_ptr=ret.ptr if ret else 0, valid_ptr=valid.ptr if valid else 0,
            gamma=gamma, lam=lam, next_step=ns, team_reward=team)
    eng.sync()
    return adv, ret, valid


def expected(tape, gamma, lam, ns, team, use):
    return model(tape["rew"], tape["val"], tape["last"], tape["term"], tape["trunc"] if use["trunc"] else None,
                 tape["fv"] if use["fv"] else None, tape["prev"] if use["prev"] else None, gamma, lam, ns, team)


def check_outputs(outs, want, what):
    for o, w, name in zip(outs, want, ("advantages", "returns", "valid")):
        if o is not None:
            o.check(w, f"{what}: {name}")


# ------------------------------------------------------------------------------------------------ 2. values on constructed tapes
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_constructed_tapes_equal_the_model_bit_for_bit(name, backend, monkeypatch):
    """every shape x both modes x truncated, final_values, prev_ended, returns and valid present or NULL x every array on a 16-byte
    boundary (the 16-byte path, where B*K allows it) or the float arrays one element behind one (the element path) x four (gamma, lambda).
    (By its measured rule rw_gae gives a lane four columns only from 64 * 1024 such lanes on: RWARE_GAE_COLUMNS=4, a hook of
    csrc/rware_hooks.h that tests/conftest.py switches on, takes the rule's place here; the rule itself is the next test's.)"""
    monkeypatch.setenv("RWARE_GAE_COLUMNS", "4")
    be = backend()
    env, eng = make_engine(be)
    T, B, N, K, team = SHAPES[name]
    tape = random_tape(np.random.default_rng(sum(map(ord, name))), T, B, N, K)
    assert (tape["term"] != 0).any() or T * B < 4
    n_cases = 0
    for off in (0, 1):
        ptrs = {k: place(be, v, off if v.dtype == f32 else 0) for k, v in tape.items()}
        for ns, has_trunc, has_fv, has_prev in itertools.product((True, False), repeat=4):
            for gamma, lam in GAMMAS:
                use = dict(trunc=has_trunc, fv=has_fv, prev=has_prev)
                want = expected(tape, gamma, lam, ns, team, use)
                for has_ret, has_valid in itertools.product((True, False), repeat=2):
                    what = (f"{name} offset {off} next_step={ns} truncated={has_trunc} final_values={has_fv} prev_ended={has_prev} "
                            f"returns={has_ret} valid={has_valid} gamma={gamma} lam={lam}")
                    outs = run_op(be, eng, ptrs, (T, B, N, K), gamma, lam, ns, team, dict(use, returns=has_ret, valid=has_valid), off)
                    check_outputs(outs, want, what)
                    n_cases += 1
    assert n_cases == 2 * 16 * 4 * 4
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("B,off,what", [(65601, 1, "65 601 one-column lanes: 256-thread workgroups, the last one not full"),
                                        (65536, 0, "65 536 columns on 16-byte boundaries: still one column a lane, the last 64-thread geometry"),
                                        (4 * 65536, 0, "65 536 lanes of four columns: the first shape on the 16-byte path"),
                                        (4 * 65537, 0, "65 537 lanes of four columns: 256-thread workgroups, the last one not full")])
def test_the_shapes_at_which_the_rule_changes_the_geometry(B, off, what, backend, monkeypatch):
    """no hook: rw_gae's own rule picks columns per lane and wavefronts per workgroup"""
    monkeypatch.delenv("RWARE_GAE_COLUMNS", raising=False)
    be = backend()
    env, eng = make_engine(be)
    T, N, K = 2, 1, 1
    tape = random_tape(np.random.default_rng(8), T, B, N, K)
    ptrs = {k: place(be, v, off if v.dtype == f32 else 0) for k, v in tape.items()}
    use = dict(trunc=True, fv=False, prev=True, returns=True, valid=True)
    outs = run_op(be, eng, ptrs, (T, B, N, K), 0.99, 0.95, True, False, use, off)
    check_outputs(outs, expected(tape, 0.99, 0.95, True, False, use), what)
    env.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_hand_built_columns(backend):
    """one column per case, T = 6, one agent: the op equals the model in both modes, and the definition's consequences hold"""
    be = backend()
    env, eng = make_engine(be)
    T, B = 6, 6
    rng = np.random.default_rng(3)
    tape = random_tape(rng, T, B, 1, 1, rate=0.0)
    term, trunc, prev = tape["term"], tape["trunc"], tape["prev"]
    prev[:] = 0
    term[2, 0] = trunc[2, 0] = 1              # column 0: both flags on one step
    trunc[T - 1, 1] = 1                       # column 1: an end on the tape's last step
    term[2, 2] = term[3, 2] = 1               # column 2: ends on consecutive steps
    term[2, 3], trunc[3, 3] = 1, 1            # column 3: under NEXT_STEP step 3 is a reset step that carries a flag
    prev[4], term[0, 4] = 1, 1                # column 4: the tape before ended, and step 0 ends again
    assert not term[:, 5].any() and not trunc[:, 5].any()   # column 5: no end at all
    ptrs = {k: place(be, v) for k, v in tape.items()}
    use = dict(trunc=True, fv=True, prev=True, returns=True, valid=True)
    g, lam = 0.99, 0.95
    for ns in (True, False):
        want = expected(tape, g, lam, ns, False, use)
        check_outputs(run_op(be, eng, ptrs, (T, B, 1, 1), g, lam, ns, False, use), want, f"hand-built next_step={ns}")
        adv, ret, valid = (w[:, :, 0] if w.ndim == 3 else w for w in want)
        val, rew, fv, last = tape["val"][:, :, 0], tape["rew"][:, :, 0], tape["fv"][:, :, 0], tape["last"][:, 0]
        one_step = lambda t, b, boot: (rew[t, b] + f32(g) * f32(boot)) - val[t, b]
        assert adv[2, 0] == one_step(2, 0, 0)                                      # terminated wins over truncated: no bootstrap
        assert adv[T - 1, 1] == one_step(T - 1, 1, last[1] if ns else fv[T - 1, 1])   # truncated on the last row: last_values / final_values
        assert adv[2, 2] == one_step(2, 2, 0)
        if ns:
            assert valid[:, 2].tolist() == [1, 1, 1, 0, 0, 1] and adv[3, 2] == 0 and adv[4, 2] == 0
            assert valid[:, 3].tolist() == [1, 1, 1, 0, 0, 1] and adv[3, 3] == 0 and ret[3, 3] == val[3, 3]   # reset beats its own flags
            assert adv[2, 3] == one_step(2, 3, 0)                                  # ... and the end in front of it saw nothing of it
            assert valid[:, 4].tolist() == [0, 0, 1, 1, 1, 1] and adv[0, 4] == 0 and adv[1, 4] == 0
        else:
            assert valid.all() and adv[3, 2] == one_step(3, 2, 0) and adv[3, 3] == one_step(3, 3, fv[3, 3])
            assert adv[0, 4] == one_step(0, 4, 0)
        assert valid[:, 5].all() and adv[T - 1, 5] == one_step(T - 1, 5, last[5])
    env.close()


# ------------------------------------------------------------------------------------------------ 3. the model against an independent computation
def test_the_model_and_the_host_function_agree_with_textbook_gae_per_episode():
    """CPU only, no engine: 300 random tapes.  valid equal; advantages within 5 * T * 2^-24 * A of the float64 per-episode computation
    (five roundings a step, see `bound`); rware_amd.gae equals the model bit for bit, in both forms of `values`."""
    rng = np.random.default_rng(2024)
    worst = 0.0
    for i in range(300):
        T, B, N = int(rng.integers(1, 17)), int(rng.integers(1, 5)), int(rng.integers(1, 5))
        K = N if rng.random() < 0.6 else 1
        team = (K == 1 and N > 1) or (K == N and rng.random() < 0.3)
        ns, gamma, lam = bool(rng.random() < 0.5), *GAMMAS[i % 4]
        tape = random_tape(rng, T, B, N, K)
        trunc = tape["trunc"] if i % 3 else None
        fv = tape["fv"] if i % 5 else None
        prev = tape["prev"] if i % 7 else None
        adv, ret, valid = model(tape["rew"], tape["val"], tape["last"], tape["term"], trunc, fv, prev, gamma, lam, ns, team)
        adv64, valid64 = episodes_f64(tape["rew"], tape["val"], tape["last"], tape["term"], trunc, fv, prev, gamma, lam, ns, team)
        assert np.array_equal(valid != 0, valid64), i
        seen = team_sum(tape["rew"]) if team else tape["rew"]
        lim = bound(T, adv64, np.concatenate([tape["val"].ravel(), tape["last"].ravel(), tape["fv"].ravel()]), seen)
        err = float(np.abs(adv.astype(np.float64) - adv64).max())
        assert err <= lim, (i, err, lim)
        worst = max(worst, err / lim)
        assert np.array_equal(ret.view(np.uint32), (adv + tape["val"]).view(np.uint32))
        # the host function, in both forms of `values`, flags as uint8 or bool
        kw = dict(truncated=trunc, final_values=fv, prev_ended=prev, gamma=gamma, lam=lam, team_reward=team, next_step=ns)
        a1, r1, v1 = rware_amd.gae(tape["rew"], tape["val"], tape["term"], last_values=tape["last"], **kw)
        stacked = np.concatenate([tape["val"], tape["last"][None]])
        kw["truncated"] = None if trunc is None else trunc != 0
        a2, r2, v2 = rware_amd.gae(tape["rew"], stacked, tape["term"] != 0, **kw)
        for got_a, got_r, got_v in ((a1, r1, v1), (a2, r2, v2)):
            assert got_a.dtype == got_r.dtype == f32 and got_v.dtype == bool
            assert np.array_equal(got_a.view(np.uint32), adv.view(np.uint32)), i
            assert np.array_equal(got_r.view(np.uint32), ret.view(np.uint32)), i
            assert np.array_equal(got_v, valid != 0), i
    print(f"worst error / bound over 300 tapes: {worst:.3f}")
    assert 0 < worst < 1


def test_the_host_function_takes_values_without_a_head_axis_and_refuses_bad_arguments():
    rng = np.random.default_rng(5)
    tape = random_tape(rng, 7, 3, 2, 1)
    want = model(tape["rew"], tape["val"], tape["last"], tape["term"], tape["trunc"], None, None, 0.99, 0.95, True, True)
    flat = np.concatenate([tape["val"], tape["last"][None]])[:, :, 0]
    a, r, v = rware_amd.gae(tape["rew"], flat, tape["term"], tape["trunc"])            # team_reward=None: K == 1 and N > 1; next_step=None: yes
    assert a.shape == r.shape == (7, 3) and v.shape == (7, 3)
    assert np.array_equal(a.view(np.uint32), want[0][:, :, 0].view(np.uint32)) and np.array_equal(v, want[2] != 0)
    outs = (np.empty((7, 3), f32), np.empty((7, 3), f32), np.empty((7, 3), bool))
    got = rware_amd.gae(tape["rew"], flat, tape["term"], tape["trunc"], out=outs)
    assert got[0] is outs[0] and np.array_equal(outs[1].view(np.uint32), want[1][:, :, 0].view(np.uint32))
    bad = {
        "float64 rewards": dict(rewards=tape["rew"].astype(np.float64)),
        "2-D rewards": dict(rewards=tape["rew"][:, :, 0]),
        "values one row short": dict(values=flat[:-1]),
        "three heads for two agents": dict(values=np.zeros((8, 3, 3), f32)),
        "int flags": dict(terminated=tape["term"].astype(np.int32)),
        "flags of another shape": dict(terminated=tape["term"][:-1]),
        "gamma above 1": dict(gamma=1.5),
        "lam below 0": dict(lam=-0.1),
        "gamma NaN": dict(gamma=float("nan")),
        "one head without the team reward": dict(team_reward=False),
    }
    for what, kw in bad.items():
        args = dict(dict(rewards=tape["rew"], values=flat, terminated=tape["term"]), **kw)
        with pytest.raises(ValueError):
            rware_amd.gae(**args)
            pytest.fail(f"{what}: accepted")


# ------------------------------------------------------------------------------------------------ 4. engine tapes
ENGINE_TAPES = dict(max_steps=4, max_inactivity_steps=3, time_limit_truncates=True)
ACTION_P = [0.05, 0.45, 0.1, 0.1, 0.3]
# With these limits an episode ends by inactivity at its third step unless a shelf is delivered within three steps of a reset, which
# random actions do not manage (no seed of 400 did, in either mode, on the emulated build): no tape would hold a truncated end.  So
# the step counters of four of the six envs are advanced after reset() — state injection, as the reference's own tests do it: envs 2
# and 3 reach max_steps at their second step (truncated only), env 4 at its third together with the inactivity limit (both flags),
# env 5 at its first (an end on step 0).  Everything after those first ends is the engine's own course under random actions.
ENGINE_STEPS = [0, 0, 2, 2, 1, 3]
# mode -> (seed, terminated-only ends, truncated ends, ends on a tape's last row), counted on the emulated build
ENGINE_SEEDS = {"next_step": (3, 17, 4, 5), "same_step": (3, 23, 4, 3)}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_engine_tapes(mode, backend):
    """two consecutive 7-step rollouts of six tiny two-agent warehouses: the tape has the properties the op relies on; the op equals the
    model and agrees with the per-episode float64 computation on each tape and on both together; the second tape chained by
    prev_ended gives rows 7 .. 13 of the 14-step result"""
    be = backend()
    B, N, T = 6, 2, 7
    seed, n_term_only, n_trunc, n_last = ENGINE_SEEDS[mode]
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1", **ENGINE_TAPES)
    env = rware_amd.WarehouseVecEnv(B, library=be.library(), autoreset_mode=mode, **dict(kw, **be.kw))
    eng = env.engines[0]
    env.reset(seed=seed)
    env.set_state(steps=np.array(ENGINE_STEPS, np.int32))
    rng = np.random.default_rng(seed)
    tapes = [env.rollout(rng.choice(5, size=(T, B, N), p=ACTION_P).astype(np.int32), want_obs=False)[1:] for _ in range(2)]
    rew, term, trunc = (np.concatenate([tp[k] for tp in tapes]) for k in range(3))
    assert rew.shape == (2 * T, B, N) and rew.dtype == f32 and term.shape == trunc.shape == (2 * T, B)
    term, trunc = term.astype(np.uint8), trunc.astype(np.uint8)
    ended = (term | trunc) != 0
    # the facts the op relies on, on the tape itself
    if mode == "next_step":
        after = ended[:-1]
        assert not ended[1:][after].any() and (rew[1:][after] == 0).all(), "the step after an end is a reset step: reward 0, no flags"
    counts = (int(((term != 0) & (trunc == 0)).sum()), int((trunc != 0).sum()), int(ended[T - 1].sum() + ended[2 * T - 1].sum()))
    assert counts == (n_term_only, n_trunc, n_last) and min(counts) >= 1, counts
    vrng = np.random.default_rng(77)
    for K, team in ((N, False), (1, True)):
        val, last, fv = (vrng.normal(size=s).astype(f32) for s in ((2 * T, B, K), (B, K), (2 * T, B, K)))
        use = dict(trunc=True, fv=True, prev=True, returns=True, valid=True)
        ns = mode == "next_step"
        whole = dict(rew=rew, val=val, last=last, fv=fv, term=term, trunc=trunc, prev=np.zeros(B, np.uint8))
        second = dict(rew=rew[T:], val=val[T:], last=last, fv=fv[T:], term=term[T:], trunc=trunc[T:], prev=ended[T - 1].astype(np.uint8))
        first = dict(rew=rew[:T], val=val[:T], last=val[T], fv=fv[:T], term=term[:T], trunc=trunc[:T], prev=np.zeros(B, np.uint8))
        results = {}
        for what, tape in (("whole", whole), ("first", first), ("second", second)):
            steps = len(tape["rew"])
            ptrs = {k: place(be, v) for k, v in tape.items()}
            outs = run_op(be, eng, ptrs, (steps, B, N, K), 0.99, 0.95, ns, team, use)
            want = expected(tape, 0.99, 0.95, ns, team, use)
            check_outputs(outs, want, f"{mode} K={K} {what}")
            adv64, valid64 = episodes_f64(tape["rew"], tape["val"], tape["last"], tape["term"], tape["trunc"], tape["fv"], tape["prev"],
                                          0.99, 0.95, ns, team)
            assert np.array_equal(want[2] != 0, valid64)
            seen = team_sum(tape["rew"]) if team else tape["rew"]
            lim = bound(steps, adv64, np.concatenate([tape["val"].ravel(), tape["last"].ravel(), tape["fv"].ravel()]), seen)
            assert float(np.abs(want[0].astype(np.float64) - adv64).max()) <= lim
            results[what] = want
        # the second tape alone, chained by prev_ended, is rows 7 .. 13 of the 14-step tape (the op equalled both models above)
        for k in range(3):
            assert np.array_equal(results["second"][k].view(np.uint8), results["whole"][k][T:].view(np.uint8)), (mode, K, k)
        if ns:
            assert ended[T - 1].any() and not results["second"][2][0][ended[T - 1]].any()
    env.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("backend", BACKENDS)
def test_each_refusal_returns_invalid_arg_names_the_argument_and_writes_nothing(backend):
    be = backend()
    env, eng = make_engine(be)
    T, B, N = 4, 3, 2
    tape = random_tape(np.random.default_rng(1), T, B, N, N)
    p = {k: place(be, v) for k, v in tape.items()}
    adv, ret, valid = Output(be, T * B * N, 4), Output(be, T * B * N, 4), Output(be, T * B, 1)
    fn, h = eng.lib.rw_gae, eng._h
    NS, TEAM = _capi.GAE_NEXT_STEP, _capi.GAE_TEAM_REWARD

    def args(**change):
        base = dict(rewards_dev=p["rew"], values_dev=p["val"], last_values_dev=p["last"], terminated_dev=p["term"], truncated_dev=p["trunc"],
                    final_values_dev=p["fv"], prev_ended_dev=p["prev"], advantages_dev=adv.ptr, returns_dev=ret.ptr, valid_dev=valid.ptr,
                    n_steps=T, n_envs=B, n_agents=N, n_heads=N, gamma=0.99, lam=0.95, flags=NS, reserved=0)
        base.update(change)
        return _capi.RwGaeArgs(**{k: (v or None) if k.endswith("_dev") else v for k, v in base.items()})

    good = args()
    assert fn(None, C.byref(good)) == INVALID and fn(h, None) == INVALID and b"args" in eng.lib.rw_last_error(h)
    refused = {  # what -> (changed fields, a word of the message)
        "NULL rewards_dev": (dict(rewards_dev=0), "rewards_dev"), "NULL values_dev": (dict(values_dev=0), "values_dev"),
        "NULL last_values_dev": (dict(last_values_dev=0), "last_values_dev"), "NULL terminated_dev": (dict(terminated_dev=0), "terminated_dev"),
        "NULL advantages_dev": (dict(advantages_dev=0), "advantages_dev"),
        "n_steps -1": (dict(n_steps=-1), "n_steps"), "n_envs -1": (dict(n_envs=-1), "n_envs"),
        "n_agents -1": (dict(n_agents=-1, n_heads=1), "n_agents"), "n_heads -1": (dict(n_heads=-1), "n_heads"),
        "n_heads 3 of 2 agents": (dict(n_heads=3), "n_heads"), "n_heads 0 of 2 agents": (dict(n_heads=0), "n_heads"),
        "one head, two agents, no team reward": (dict(n_heads=1), "RW_GAE_TEAM_REWARD"),
        "flag bit 4": (dict(flags=NS | 4), "flag"), "flag bit 31": (dict(flags=-2**31), "flag"), "reserved 1": (dict(reserved=1), "reserved"),
        "gamma 1.5": (dict(gamma=1.5), "gamma"), "gamma -0.1": (dict(gamma=-0.1), "gamma"), "gamma NaN": (dict(gamma=float("nan")), "gamma"),
        "gamma inf": (dict(gamma=float("inf")), "gamma"), "lam 1.0001": (dict(lam=1.0001), "lam"), "lam -1": (dict(lam=-1.0), "lam"),
        "lam NaN": (dict(lam=float("nan")), "lam"), "lam -inf": (dict(lam=float("-inf")), "lam"),
        "rewards_dev at 2 bytes": (dict(rewards_dev=p["rew"] + 2), "rewards_dev"), "values_dev at 1 byte": (dict(values_dev=p["val"] + 1), "values_dev"),
        "last_values_dev at 2 bytes": (dict(last_values_dev=p["last"] + 2), "last_values_dev"),
        "final_values_dev at 2 bytes": (dict(final_values_dev=p["fv"] + 2, flags=0), "final_values_dev"),
        "advantages_dev at 2 bytes": (dict(advantages_dev=adv.ptr + 2), "advantages_dev"),
        "returns_dev at 3 bytes": (dict(returns_dev=ret.ptr + 3), "returns_dev"),
        "advantages on values": (dict(advantages_dev=p["val"]), "overlaps"), "advantages on returns": (dict(advantages_dev=ret.ptr), "overlaps"),
        "returns on the tail of rewards": (dict(returns_dev=p["rew"] + 4 * (T * B * N - 1)), "overlaps"),
        "returns on last_values": (dict(returns_dev=p["last"]), "overlaps"),
        "advantages on final_values, which the mode reads": (dict(advantages_dev=p["fv"], flags=0), "overlaps"),
        "valid on terminated": (dict(valid_dev=p["term"]), "overlaps"), "valid on truncated": (dict(valid_dev=p["trunc"] + T * B - 1), "overlaps"),
        "valid on prev_ended": (dict(valid_dev=p["prev"]), "overlaps"), "valid inside advantages": (dict(valid_dev=adv.ptr + 5), "overlaps"),
        "2^32 columns": (dict(n_envs=2**30, n_agents=4, n_heads=4), "slices of envs"),
        "2^31 rewards a step": (dict(n_envs=2**24, n_agents=128, n_heads=1, flags=NS | TEAM), "slices of envs"),
        "2^40 elements": (dict(n_steps=2**20, n_envs=2**20, n_agents=1, n_heads=1), "slices of envs"),
    }
    for what, (change, word) in refused.items():
        assert fn(h, C.byref(args(**change))) == INVALID, what
        msg = eng.lib.rw_last_error(h).decode()
        assert "rw_gae" in msg and word in msg, (what, msg)
    assert eng.lib.rw_sync(h) == OK
    for o in (adv, ret, valid):
        o.untouched("refusals")
    # what a mode does not read is not looked at: a misaligned or overlapping pointer there is no error
    # (NEXT_STEP ignores final_values_dev, the other mode prev_ended_dev) — but nothing may be written through them either
    for change in (dict(n_steps=0), dict(n_envs=0), dict(n_steps=0, n_envs=0), dict(n_agents=0, n_heads=0)):
        assert fn(h, C.byref(args(**change))) == OK, change
    assert eng.lib.rw_sync(h) == OK
    for o in (adv, ret, valid):
        o.untouched("an empty tape")
    use = dict(trunc=True, fv=True, prev=True, returns=True, valid=True)
    assert fn(h, C.byref(args(final_values_dev=adv.ptr + 2))) == OK                # NEXT_STEP: final_values_dev is not looked at
    assert eng.lib.rw_sync(h) == OK
    check_outputs((adv, ret, valid), expected(tape, 0.99, 0.95, True, False, dict(use, fv=False)), "ignored final_values_dev")
    assert fn(h, C.byref(args(prev_ended_dev=valid.ptr, flags=0))) == OK           # the other mode: prev_ended_dev is not looked at
    assert eng.lib.rw_sync(h) == OK
    check_outputs((adv, ret, valid), expected(tape, 0.99, 0.95, False, False, dict(use, prev=False)), "ignored prev_ended_dev")
    env.close()


# ------------------------------------------------------------------------------------------------ 6. the torch surface
def torch_env(B=6, mode="next_step", **more):
    kw = lockstep.oracle_kwargs("rware-tiny-2ag-v1", **ENGINE_TAPES)
    return rware_amd.WarehouseVecEnv(B, output="torch", autoreset_mode=mode, **dict(kw, **more))


def torch_tape(env, T, seed):
    import torch

    env.reset(seed=seed)
    actions = torch.from_numpy(np.random.default_rng(seed).choice(5, size=(T, env.num_envs, env.n_agents), p=ACTION_P).astype(np.int32)).cuda()
    _, rew, term, trunc = env.rollout(actions, want_obs=False)
    return rew, term, trunc


def same_bits(got, want, what):
    for g, w, name in zip(got, want, ("advantages", "returns", "valid")):
        g = g.cpu().numpy()
        w = w.reshape(g.shape)
        assert g.dtype == (bool if name == "valid" else f32), (what, name, g.dtype)
        assert np.array_equal(g.view(np.uint8), (w != 0).view(np.uint8) if name == "valid" else w.view(np.uint8)), f"{what}: {name}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_gae_device_equals_the_model_on_rollout_tapes(mode):
    import torch

    T = 9
    env = torch_env(mode=mode)
    B, N = env.num_envs, env.n_agents
    rew, term, trunc = torch_tape(env, T, seed=5)
    assert rew.is_cuda and term.dtype == trunc.dtype == torch.bool and (term | trunc).any()
    ns = mode == "next_step"
    rng = np.random.default_rng(9)
    h = dict(rew=rew.cpu().numpy(), term=term.cpu().numpy().astype(np.uint8), trunc=trunc.cpu().numpy().astype(np.uint8))
    for K in (N, 1):
        val, last, fv = (rng.normal(size=s).astype(f32) for s in ((T, B, K), (B, K), (T, B, K)))
        prev = (rng.random(B) < 0.5).astype(np.uint8)
        stacked = torch.from_numpy(np.concatenate([val, last[None]])).cuda()
        want = model(h["rew"], val, last, h["term"], h["trunc"], None if ns else fv, prev if ns else None, 0.99, 0.95, ns, K == 1)
        d = lambda a: torch.from_numpy(a).cuda()
        # values (T+1, B, K), bool flags; the mode from the env; team_reward from the shapes
        got = env.gae_device(rew, stacked, term, trunc, final_values=d(fv), prev_ended=d(prev).view(torch.bool))
        env.sync()
        same_bits(got, want, f"{mode} K={K} stacked")
        again = env.gae_device(rew, stacked, term, trunc, final_values=d(fv), prev_ended=d(prev).view(torch.bool))
        assert all(a is b for a, b in zip(got, again)), "the cached outputs are the same objects on a second call"
        # values (T, B, K) with last_values, uint8 flags, the mode and the reward spelled out
        got = env.gae_device(rew, d(val), term.view(torch.uint8), trunc.view(torch.uint8), last_values=d(last), final_values=d(fv),
                             prev_ended=d(prev), next_step=ns, team_reward=K == 1)
        env.sync()
        same_bits(got, want, f"{mode} K={K} last_values")
        if K == 1:                                                   # ... and without a head axis
            got = env.gae_device(rew, stacked[:, :, 0].contiguous(), term, trunc, final_values=d(fv[:, :, 0].copy()), prev_ended=d(prev))
            env.sync()
            assert tuple(got[0].shape) == tuple(got[1].shape) == (T, B)
            same_bits(got, want, f"{mode} K=1 flat")
        # out=: slices of larger buffers
        big_a, big_r = torch.full((3, T, B, K), 7.0, device="cuda"), torch.full((T + 2, B, K), 7.0, device="cuda")
        big_v = torch.ones((2, T, B), dtype=torch.bool, device="cuda")
        outs = (big_a[1], big_r[1:T + 1], big_v[1])
        got = env.gae_device(rew, stacked, term, trunc, final_values=d(fv), prev_ended=d(prev), out=outs)
        env.sync()
        assert all(a is b for a, b in zip(got, outs))
        same_bits(got, want, f"{mode} K={K} out=")
        assert (big_a[0] == 7).all() and (big_a[2] == 7).all() and (big_r[0] == 7).all() and (big_r[T + 1] == 7).all() and big_v[0].all()
    env.close()


@pytest.mark.gpu
def test_gae_device_refuses_bad_arguments_with_value_error():
    import torch

    T = 5
    env = torch_env()
    B, N = env.num_envs, env.n_agents
    rew, term, trunc = torch_tape(env, T, seed=2)
    val = torch.zeros((T + 1, B, N), device="cuda")
    fine = dict(rewards=rew, values=val, terminated=term, truncated=trunc)
    env.gae_device(**fine)
    env.sync()
    z = lambda *s, **k: torch.zeros(s, device="cuda", **k)
    bad = {
        "host rewards": dict(rewards=rew.cpu(), values=val.cpu(), terminated=term.cpu(), truncated=None),
        "host values": dict(values=val.cpu()),
        "host flags": dict(terminated=term.cpu()),
        "numpy tapes": dict(rewards=rew.cpu().numpy(), values=val.cpu().numpy(), terminated=term.cpu().numpy(), truncated=None),
        "2-D rewards": dict(rewards=rew[:, :, 0].contiguous()),
        "values one row short": dict(values=val[:T]),
        "values of another batch": dict(values=z(T + 1, B + 1, N)),
        "three heads for two agents": dict(values=z(T + 1, B, 3)),
        "last_values of another shape": dict(values=val[:T], last_values=z(B)),
        "float64 rewards": dict(rewards=rew.double()),
        "float16 values": dict(values=val.half()),
        "int32 flags": dict(terminated=term.to(torch.int32)),
        "float truncated": dict(truncated=trunc.float()),
        "flags of another shape": dict(terminated=term[:-1]),
        "prev_ended of another shape": dict(prev_ended=z(B + 1, dtype=torch.bool)),
        "final_values of another shape": dict(final_values=z(T, B), next_step=False),
        "non-contiguous rewards": dict(rewards=z(T, N, B).transpose(1, 2)),
        "sliced values": dict(values=z(T + 1, B, 2 * N)[:, :, :N]),
        "transposed flags": dict(terminated=z(B, T, dtype=torch.bool).t()),
        "out of two": dict(out=(z(T, B, N), z(T, B, N))),
        "out: advantages of another shape": dict(out=(z(T, B), z(T, B, N), z(T, B, dtype=torch.bool))),
        "out: returns of another dtype": dict(out=(z(T, B, N), z(T, B, N, dtype=torch.float64), z(T, B, dtype=torch.bool))),
        "out: valid as uint8": dict(out=(z(T, B, N), z(T, B, N), z(T, B, dtype=torch.uint8))),
        "out: valid on the host": dict(out=(z(T, B, N), z(T, B, N), torch.zeros((T, B), dtype=torch.bool))),
        "out: advantages on another device": dict(out=(torch.zeros((T, B, N), device="meta"), z(T, B, N), z(T, B, dtype=torch.bool))),
        "out: non-contiguous returns": dict(out=(z(T, B, N), z(T, B, 2 * N)[:, :, :N], z(T, B, dtype=torch.bool))),
        "gamma above 1": dict(gamma=1.01), "gamma below 0": dict(gamma=-0.5), "lam above 1": dict(lam=2), "lam NaN": dict(lam=float("nan")),
        "one head without the team reward": dict(values=z(T + 1, B), team_reward=False),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            env.gae_device(**dict(fine, **kw))
            pytest.fail(f"{what}: accepted")
    env.sync()
    env.close()
    numpy_env = rware_amd.WarehouseVecEnv(2, **lockstep.oracle_kwargs("rware-tiny-2ag-v1"))
    with pytest.raises(ValueError):
        numpy_env.gae_device(rew[:, :2].contiguous(), val[:, :2].contiguous(), term[:, :2].contiguous())
    numpy_env.close()


@pytest.mark.gpu
def test_a_captured_call_reads_the_tensors_at_every_replay():
    """one captured kernel on the env's stream; a host synchronisation, an allocation or a host read inside the capture would fail it"""
    import torch

    T = 6
    env = torch_env()
    B, N = env.num_envs, env.n_agents
    rew, term, trunc = torch_tape(env, T, seed=11)
    env.sync()
    val, prev = torch.zeros((T + 1, B, N), device="cuda"), torch.zeros(B, dtype=torch.bool, device="cuda")
    outs = (torch.zeros((T, B, N), device="cuda"), torch.zeros((T, B, N), device="cuda"), torch.zeros((T, B), dtype=torch.bool, device="cuda"))
    call = lambda: env.gae_device(rew, val, term, trunc, prev_ended=prev, gamma=0.9, lam=0.8, out=outs)
    call()                                                                           # (warm-up outside the capture)
    env.sync()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    env.set_stream(stream) if hasattr(env, "set_stream") else [e.set_stream(stream.cuda_stream) for e in env.engines]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            call()
    rng = np.random.default_rng(4)
    for rep in range(2):
        h = dict(rew=rng.normal(size=(T, B, N)).astype(f32), val=rng.normal(size=(T + 1, B, N)).astype(f32),
                 term=(rng.random((T, B)) < 0.2).astype(np.uint8), trunc=(rng.random((T, B)) < 0.2).astype(np.uint8),
                 prev=(rng.random(B) < 0.5).astype(np.uint8))
        with torch.cuda.stream(stream):
            rew.copy_(torch.from_numpy(h["rew"]))
            val.copy_(torch.from_numpy(h["val"]))
            term.copy_(torch.from_numpy(h["term"]).bool())
            trunc.copy_(torch.from_numpy(h["trunc"]).bool())
            prev.copy_(torch.from_numpy(h["prev"]).bool())
            for o in outs:
                o.zero_()
            graph.replay()
        stream.synchronize()
        want = model(h["rew"], h["val"][:T], h["val"][T], h["term"], h["trunc"], None, h["prev"], 0.9, 0.8, True, False)
        same_bits(outs, want, f"replay {rep}")
    env.close()


def _two_devices():
    import torch   # (a broken import fails the collection: it is no reason to skip)

    return torch.cuda.device_count() >= 2


@pytest.mark.gpu
@pytest.mark.skipif(not _two_devices(), reason="one GPU visible: a sharded env needs two")
def test_a_sharded_envs_second_device_picks_its_own_engine():
    import torch

    env = rware_amd.WarehouseVecEnv(8, output="torch", devices=[0, 1], **lockstep.oracle_kwargs("rware-tiny-2ag-v1"))
    T, B, N = 4, 5, 2
    rng = np.random.default_rng(6)
    for dev in (0, 1):
        tape = random_tape(rng, T, B, N, N)
        d = lambda a: torch.from_numpy(a).to(f"cuda:{dev}")
        got = env.gae_device(d(tape["rew"]), d(tape["val"]), d(tape["term"]), d(tape["trunc"]), last_values=d(tape["last"]), prev_ended=d(tape["prev"]))
        env.sync()
        assert all(g.device.index == dev for g in got)
        same_bits(got, model(tape["rew"], tape["val"], tape["last"], tape["term"], tape["trunc"], None, tape["prev"], 0.99, 0.95, True, False),
                  f"device {dev}")
    env.close()
