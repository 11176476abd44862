"""Constructed PCG64 states: generator states built so that the NEXT draws take a chosen branch of numpy's bounded draw
(`random_bounded_uint64` -> `buffered_bounded_lemire_uint32`) — a rejection, a threshold boundary, an extreme result — instead of
waiting for seeded play to reach it (for n = 47 a rejection needs one of 42 values out of 2^32).

How a state is built.  PCG64 is the LCG `state' = state * MULT + inc (mod 2^128)` with the XSL-RR output of the POST-step state:
`rotr64(hi ^ lo, hi >> 58)`.  The step is invertible (`state = (state' - inc) * MULT^-1`), so a post-state with a chosen output is
written down directly — `hi` with the wanted rotation in its top six bits, `lo = hi ^ rotl64(output, rot)` — and stepped back once:
the pre-state's next 64-bit output is the chosen value.  `has_uint32 = 1, uinteger = u` puts a third chosen 32-bit value in front.
Stepping back further (`back` more inverse steps) moves the chosen output behind `back` ordinary 64-bit draws: that is how a draw in
the middle of `reset()` is reached.

Three chosen 32-bit values in a row (the buffered half, then the low and the high half of one 64-bit output) are the most that
inversion can force: the output after that is a function of the state already fixed.  Nothing here searches for more.

A state is six uint64 words in RW_BUF_RNG field order: state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger.

`Tracer` is a plain-Python restatement of numpy's draws that also RECORDS what every draw did (redraws, whether the outer `if` was
entered), so a test can assert that a constructed state takes the branch it claims — a condition on the inputs, decided on the CPU.
"""
from collections import namedtuple

import numpy as np

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
MULT = 0x2360ED051FC65DA44385DF649FCCF645
MULT_INV = pow(MULT, -1, 1 << 128)
assert (MULT * MULT_INV) & M128 == 1

# bounds (exclusive) every builder is run for: the S - Q and HW - N + j values of the tasks of tests/golden/rng_edges, and two
# powers of two (threshold == 0: no draw can be rejected)
BOUNDS = (3, 5, 6, 7, 28, 30, 47, 76, 109, 110, 140, 221)
POW2_BOUNDS = (4, 32)


# ------------------------------------------------------------------------------------------------------------ words <-> integers
def words(state, inc, has_uint32=0, uinteger=0):
    return np.array([state >> 64, state & M64, inc >> 64, inc & M64, has_uint32, uinteger], dtype=np.uint64)


def unwords(w):
    w = [int(v) for v in w]
    return (w[0] << 64) | w[1], (w[2] << 64) | w[3], w[4], w[5]


def numpy_state(w):
    """The dict `Generator.bit_generator.state` takes."""
    s, inc, has, u = unwords(w)
    return {"bit_generator": "PCG64", "state": {"state": s, "inc": inc}, "has_uint32": has, "uinteger": u}


def numpy_generator(w):
    g = np.random.Generator(np.random.PCG64(0))
    g.bit_generator.state = numpy_state(w)
    return g


def words_of_numpy(gen):
    st = gen.bit_generator.state
    return words(st["state"]["state"], st["state"]["inc"], st["has_uint32"], st["uinteger"])


def real_inc(seed):
    """The increment numpy derives from SeedSequence(seed): always odd."""
    inc = np.random.PCG64(np.random.SeedSequence(seed)).state["state"]["inc"]
    assert inc & 1
    return inc


# ------------------------------------------------------------------------------------------------------------ the LCG, both ways
def step(state, inc):
    return (state * MULT + inc) & M128


def step_back(state, inc, times=1):
    for _ in range(times):
        state = ((state - inc) * MULT_INV) & M128
    return state


def output(state):
    """XSL-RR 128/64 of a POST-step state."""
    hi, lo = state >> 64, state & M64
    x, rot = hi ^ lo, hi >> 58
    return ((x >> rot) | (x << ((64 - rot) & 63))) & M64


def post_state_with_output(out64, rot=0, filler=0x2545F4914F6CDD1D):
    """A post-step state whose output is `out64`, with rotation `rot` (0..63); `filler` fills the 58 free bits of the high word."""
    hi = (rot << 58) | (filler & ((1 << 58) - 1))
    x = ((out64 << rot) | (out64 >> ((64 - rot) & 63))) & M64 if rot else out64
    st = (hi << 64) | (hi ^ x)
    assert output(st) == out64 and st >> 122 == rot
    return st


def state_before_output(out64, inc, rot=0, back=0, filler=0x2545F4914F6CDD1D):
    """The state from which the (back + 1)-th next 64-bit output is `out64`."""
    return step_back(post_state_with_output(out64, rot, filler), inc, back + 1)


# ------------------------------------------------------------------------------------------------------------ the traced draws
Draw = namedtuple("Draw", "n value redraws entered")   # bound (exclusive), result, rejected 32-bit values, outer `if` entered


class Tracer:
    """numpy's PCG64 next_uint32 / bounded draw / choice(replace=False) in Python integers, with a record per bounded draw."""

    def __init__(self, w):
        self.state, self.inc, self.has, self.u = unwords(w)
        self.draws = []
        self.n64 = 0        # 64-bit outputs consumed

    def words(self):
        return words(self.state, self.inc, self.has, self.u)

    def next64(self):
        self.state = step(self.state, self.inc)
        self.n64 += 1
        return output(self.state)

    def next32(self):
        if self.has:
            self.has = 0
            return self.u
        v = self.next64()
        self.has, self.u = 1, v >> 32
        return v & 0xFFFFFFFF

    def bounded(self, rng):
        """Uniform in [0, rng] — numpy's argument convention; the bound of the record is rng + 1."""
        if rng == 0:
            self.draws.append(Draw(1, 0, 0, False))
            return 0
        n = rng + 1
        m = self.next32() * n
        redraws, entered = 0, False
        if (m & 0xFFFFFFFF) < n:
            entered = True
            threshold = (0xFFFFFFFF - rng) % n
            while (m & 0xFFFFFFFF) < threshold:
                m = self.next32() * n
                redraws += 1
        self.draws.append(Draw(n, m >> 32, redraws, entered))
        return m >> 32

    def choice(self, pop, k):
        """Generator.choice(pop, size=k, replace=False) for pop <= 10000: Floyd, then the Fisher-Yates pass."""
        out = []
        for j in range(pop - k, pop):
            v = self.bounded(j)
            out.append(j if v in out else v)
        for i in range(k - 1, 0, -1):
            j = self.bounded(i)
            out[i], out[j] = out[j], out[i]
        return out

    def reset(self, HW, N, S, Q):
        """The draws of Warehouse.reset in order: agent cells, directions, request queue (ids from 1)."""
        cells = self.choice(HW, N)
        dirs = [self.bounded(3) for _ in range(N)]
        queue = [v + 1 for v in self.choice(S, Q)]
        return cells, dirs, queue


def trace_bounded(w, n):
    """(value, redraws, entered_outer_if, end state words) of one draw with exclusive bound n from state words w."""
    t = Tracer(w)
    v = t.bounded(n - 1)
    d = t.draws[-1]
    return v, d.redraws, d.entered, t.words()


# ------------------------------------------------------------------------------------------------------------ 32-bit values by effect
def threshold(n):
    return (1 << 32) % n


def granule(n):
    """Leftovers (v * n mod 2^32) are multiples of gcd(n, 2^32): for an odd n every leftover occurs, for n = 2^a * b only multiples
    of 2^a.  The threshold 2^32 mod n is such a multiple, so `threshold - granule` is the largest rejected leftover (threshold - 1
    for odd n) and exists whenever threshold > 0."""
    return n & -n


def draws_with_leftover(n, t):
    """Every 32-bit v with (v * n) mod 2^32 == t, ascending."""
    g = granule(n)
    if t % g:
        return []
    a = g.bit_length() - 1
    mod = 1 << (32 - a)
    v0 = ((t >> a) * pow(n >> a, -1, mod)) % mod
    return [v0 + k * mod for k in range(g)]


def rejected_value(n, which=0):
    """A 32-bit value the bound n rejects (leftover < threshold); `which` picks among the threshold / granule leftovers."""
    thr, g = threshold(n), granule(n)
    assert thr > 0, f"{n} is a power of two: nothing is rejected"
    t = (which % (thr // g)) * g
    v = draws_with_leftover(n, t)[which % g]
    assert (v * n) & 0xFFFFFFFF < thr
    return v


def accepted_value(n, value):
    """A 32-bit value in the middle of the range that yields `value` under bound n: leftover >= n, outer `if` not entered."""
    lo = -((-value << 32) // n)             # ceil(value * 2^32 / n)
    hi = -((-(value + 1) << 32) // n) - 1
    v = (lo + hi) // 2
    assert (v * n) >> 32 == value and ((v * n) & 0xFFFFFFFF) >= n, (n, value)
    return v


# ------------------------------------------------------------------------------------------------------------ cases
# name; exclusive bound; state words; claimed redraws; claimed `entered`; claimed value (None: whatever comes); claimed number of
# 64-bit outputs consumed (None: not claimed)
Case = namedtuple("Case", "name n state redraws entered value n64")


def _state(inc, has, u, lo, hi, rot=0, back=0):
    return words(state_before_output((hi << 32) | lo, inc, rot, back), inc, has, u)


def bounded_cases(n, inc):
    """Every builder for the exclusive bound n.  For a power of two the `reject_*` states hold the values that every other bound
    rejects most readily (leftover 0) and claim that nothing is rejected."""
    thr, g = threshold(n), granule(n)
    mid = accepted_value(n, n // 2)
    out = []
    if thr:
        r0, r1, r2 = rejected_value(n, 0), rejected_value(n, 1), rejected_value(n, 2)
        out += [
            Case("reject_buffered", n, _state(inc, 1, r0, mid, 0x12345678), 1, True, n // 2, 1),
            Case("reject_low", n, _state(inc, 0, 0, r1, mid), 1, True, n // 2, 1),
            # two / three rejections, then the next 64-bit output as it comes (its value is not chosen: see the module text)
            Case("reject_both_halves", n, _state(inc, 0, 0, r0, r1), 2, True, None, 2),
            Case("reject_three", n, _state(inc, 1, r2, r0, r1), 3, True, None, 2),
            Case("reject_three_rot63", n, _state(inc, 1, r0, r1, r2, rot=63), 3, True, None, 2),
            Case("leftover_eq_threshold", n, _state(inc, 0, 0, draws_with_leftover(n, thr)[0], 0), 0, True, None, 1),
            Case("leftover_below_threshold", n, _state(inc, 0, 0, draws_with_leftover(n, thr - g)[-1], mid), 1, True, n // 2, 1),
        ]
    else:
        z = 0   # leftover 0: rejected by every bound that rejects anything
        out += [
            Case("reject_buffered", n, _state(inc, 1, z, mid, 0x12345678), 0, True, 0, 0),
            Case("reject_low", n, _state(inc, 0, 0, z, mid), 0, True, 0, 1),
            Case("reject_both_halves", n, _state(inc, 0, 0, z, z), 0, True, 0, 1),
            Case("reject_three", n, _state(inc, 1, z, z, z), 0, True, 0, 0),
            Case("reject_three_rot63", n, _state(inc, 1, z, z, z, rot=63), 0, True, 0, 0),
        ]
    top = draws_with_leftover(n, n - g)
    out += [
        # threshold <= leftover < n: the outer `if` is entered, the loop is not
        Case("leftover_in_if_no_loop", n, _state(inc, 0, 0, top[0], 0), 0, True, (top[0] * n) >> 32, 1),
        Case("leftover_eq_n", n, _state(inc, 0, 0, 1, 0), 0, False, 0, 1),                    # 1 * n: leftover == n, value 0
        Case("value_0", n, _state(inc, 1, accepted_value(n, 0), 0, 0), 0, False, 0, 0),
        Case("value_n_minus_1", n, _state(inc, 0, 0, 0xFFFFFFFF, 0), 0, False, n - 1, 1),
        Case("uinteger_all_ones", n, _state(inc, 1, 0xFFFFFFFF, 0, 0), 0, False, n - 1, 0),
        Case("rot_0", n, _state(inc, 0, 0, mid, 0, rot=0), 0, False, n // 2, 1),
        Case("rot_63", n, _state(inc, 0, 0, mid, 0, rot=63), 0, False, n // 2, 1),
        Case("rot_1", n, _state(inc, 0, 0, mid, 0, rot=1), 0, False, n // 2, 1),
        # pre-states at the carry edges of the 128-bit multiply-add: the result is whatever numpy gives
        Case("pre_state_0", n, words(0, inc), None, None, None, None),
        Case("pre_state_all_ones", n, words(M128, inc), None, None, None, None),
        Case("pre_state_lo_all_ones", n, words((0x0123456789ABCDEF << 64) | M64, inc, 1, 0xFFFFFFFF), None, None, None, None),
        Case("pre_state_hi_0", n, words(0xFEDCBA9876543210, inc), None, None, None, None),
        Case("pre_state_lo_0", n, words(0xFEDCBA9876543210 << 64, inc), None, None, None, None),
        # (hi == lo: the output is 0 — both halves of it are rejected by every bound with a threshold)
        Case("post_state_0", n, words(step_back(0, inc), inc), 2 if thr else 0, True, None, None),
        Case("post_state_all_ones", n, words(step_back(M128, inc), inc), 2 if thr else 0, True, None, None),
    ]
    return out


def n1_case(inc):
    """n == 1 (rng == 0): nothing is consumed, the buffered half stays."""
    return Case("n_1_keeps_buffer", 1, _state(inc, 1, 0xDEADBEEF, 7, 9), 0, False, 0, 0)


# ------------------------------------------------------------------------------------------------------------ choice(pop, k)
# claim: {draw index: (redraws, entered)} of the draws the state was built for; `collide`: the Floyd slot that must take j
ChoiceCase = namedtuple("ChoiceCase", "name pop k state claim collide")
# A claimed number of redraws is exact (an int) wherever the builder chooses the value that follows the last rejected one.  Where that
# value is the next 64-bit output — the rejected one was a high half, or the third forced value — inversion does not choose it (see the
# module text) and it may reject again, with probability threshold / 2^32 per half: the claim is then AtLeast(k).
AtLeast = namedtuple("AtLeast", "n")


def redraws_as_claimed(got, claimed):
    return got >= claimed.n if isinstance(claimed, AtLeast) else got == claimed


def takes_high_half(bounds, t):
    """Whether draw t of a sequence with these bounds takes the high half of its output (has_uint32 == 0, no rejection before it)."""
    return bool([i for i, b in enumerate(bounds) if b > 1].index(t) & 1)


def choice_cases(pop, k, inc):
    """States for Generator.choice(pop, k, replace=False), k >= 2.  Draw t (0-based) of the call has exclusive bound pop - k + t + 1
    for the k Floyd draws, then k, k - 1, .. 2 for the Fisher-Yates pass; with has_uint32 == 0 and no rejection before it, draw t
    is the low (t even) or high (t odd) half of 64-bit output t // 2 — a draw with bound 1 (pop == k: Floyd's j == 0) consumes nothing."""
    assert 2 <= k <= pop
    bounds = [pop - k + t + 1 for t in range(k)] + list(range(k, 1, -1))
    out = []
    # Floyd: the second draw repeats the first one's value -> out[1] = j
    b0, b1 = bounds[0], bounds[1]
    v = b0 // 2
    if b0 > 1:
        out.append(ChoiceCase("floyd_collision", pop, k, _state(inc, 1, accepted_value(b0, v), accepted_value(b1, v), 0), {}, 1))
    else:   # pop == k: the first draw consumes nothing and yields 0; the second one (bound 2) yields 0 again
        out.append(ChoiceCase("floyd_collision", pop, k, _state(inc, 1, accepted_value(b1, 0), 0, 0), {}, 1))

    def at(t, lo_or_hi_value, other=0x7FFFFFFF):
        """State in which draw t is `lo_or_hi_value`; the other half of that output, 2^31 - 1, is accepted by every bound below 2^30
        (its leftover is 2^32 - n for an even n, 2^31 - n for an odd one)."""
        consuming = [i for i, b in enumerate(bounds) if b > 1]
        pos = consuming.index(t)
        half, back = pos & 1, pos >> 1
        lo, hi = (other, lo_or_hi_value) if half else (lo_or_hi_value, other)
        return _state(inc, 0, 0, lo, hi, back=back)

    # a rejection at the first Floyd draw that can reject, and at the first Fisher-Yates draw that can
    for name, rng_t in (("floyd_rejection", range(k)), ("fisher_yates_rejection", range(k, len(bounds)))):
        for t in rng_t:
            if threshold(bounds[t]):
                # (low half: `other`, which every bound accepts, follows; high half: the next output follows)
                out.append(ChoiceCase(name, pop, k, at(t, rejected_value(bounds[t])), {t: (AtLeast(1) if takes_high_half(bounds, t) else 1, True)}, None))
                break
    return out


def check_choice_claim(case):
    """Runs the tracer over the case and asserts its claim; returns (values, end state words)."""
    t = Tracer(case.state)
    vals = t.choice(case.pop, case.k)
    for i, (redraws, entered) in case.claim.items():
        d = t.draws[i]
        assert redraws_as_claimed(d.redraws, redraws) and d.entered == entered, (case.name, case.pop, case.k, i, d)
    if case.collide is not None:
        d0, d1 = t.draws[0], t.draws[1]
        assert d0.value == d1.value, (case.name, case.pop, case.k, d0, d1)
    return vals, t.words()


# ------------------------------------------------------------------------------------------------------------ scenarios of the fixture
# tests/golden/rng_edges/<task>.npz: name -> (registered id, constructor overrides; reward_type as its integer value).  The two custom
# shapes: a 3 x 4 layout with two goals, 4 shelves and 3 requests (S - Q == 1: the replacement draw consumes nothing), and the tiny
# warehouse with 3 requests (S - Q == 29, a prime).  9 and 16 agents are there for the kernels that keep their agent phase in LDS.
TASKS = {
    "tiny-2ag": ("rware-tiny-2ag-v2", {}),
    "small-4ag": ("rware-small-4ag-v2", {}),
    "tiny-4ag-easy": ("rware-tiny-4ag-easy-v2", {}),
    "one-candidate": ("rware-tiny-2ag-v2", dict(layout=".xx.\n.xx.\n.gg.", n_agents=3, request_queue_size=3, reward_type=0)),
    "prime-candidates": ("rware-tiny-2ag-v2", dict(n_agents=3, request_queue_size=3, reward_type=2)),
    "tiny-9ag": ("rware-tiny-9ag-v2", {}),
    "small-16ag": ("rware-small-16ag-v2", {}),
}
SAFE = 0x7FFFFFFF   # a 32-bit value every bound below 2^30 accepts without entering the outer `if`


def reset_bounds(HW, N, S, Q):
    """Exclusive bound of every draw of Warehouse.reset, in order."""
    def choice(pop, k):
        return [pop - k + t + 1 for t in range(k)] + list(range(k, 1, -1))
    return choice(HW, N) + [4] * N + choice(S, Q)


def state_at(bounds, t, inc, values):
    """A state (has_uint32 == 0) in which draw t of a sequence with these bounds sees `values` (1 .. 3 32-bit values) one after the
    other, provided no earlier draw rejects; when draw t is the low half of an output only two values can be chosen."""
    pos = [i for i, b in enumerate(bounds) if b > 1].index(t)
    half, back = pos & 1, pos >> 1
    if half:        # draw t takes the high half of output `back`: only that value is chosen (the low half went to draw t - 1)
        lo, hi = SAFE, values[0]
    else:
        lo, hi = values[0], values[1] if len(values) > 1 else SAFE
    return _state(inc, 0, 0, lo, hi, back=back)


ResetScenario = namedtuple("ResetScenario", "name claim state draws")    # draws: {draw index: (redraws, entered, value or None)}


def reset_scenarios(HW, N, S, Q, inc):
    b = reset_bounds(HW, N, S, Q)
    out = []

    def add(name, claim, state, draws):
        out.append(ResetScenario(name, claim, state, draws))

    def first_rejecting(rng_t):
        return next((t for t in rng_t if threshold(b[t])), None)

    def once(t):    # one rejected value at draw t through state_at: SAFE follows a low half, the next output a high half
        return AtLeast(1) if takes_high_half(b, t) else 1

    n0 = b[0]
    if threshold(n0):
        r = [rejected_value(n0, k) for k in range(3)]
        mid = accepted_value(n0, n0 // 2)
        add("cell_first_rejects_low", "draw 0 rejects the low half, accepts the high half", _state(inc, 0, 0, r[0], mid), {0: (1, True, n0 // 2)})
        add("cell_first_rejects_buffered", "draw 0 rejects the buffered half", _state(inc, 1, r[1], mid, SAFE), {0: (1, True, n0 // 2)})
        add("cell_first_rejects_three", "draw 0 rejects buffered, low and high half", _state(inc, 1, r[0], r[1], r[2]), {0: (AtLeast(3), True, None)})
        g, thr = granule(n0), threshold(n0)
        add("cell_first_leftover_eq_threshold", "draw 0: leftover == threshold, accepted", _state(inc, 0, 0, draws_with_leftover(n0, thr)[0], SAFE),
            {0: (0, True, None)})
        add("cell_first_leftover_below_threshold", "draw 0: the largest rejected leftover", _state(inc, 0, 0, draws_with_leftover(n0, thr - g)[-1], mid),
            {0: (1, True, n0 // 2)})
    add("cell_first_value_max", "draw 0 yields n - 1 from 0xFFFFFFFF in the buffer", _state(inc, 1, 0xFFFFFFFF, SAFE, SAFE), {0: (0, False, n0 - 1)})
    add("cell_first_value_0", "draw 0 yields 0 (leftover == n)", _state(inc, 0, 0, 1, SAFE), {0: (0, False, 0)})
    if N >= 2:
        v = n0 // 3
        add("cell_floyd_collision", "draws 0 and 1 yield the same cell: the second agent takes j", _state(inc, 1, accepted_value(n0, v), accepted_value(b[1], v), SAFE),
            {0: (0, False, v), 1: (0, False, v)})
        t = first_rejecting(range(N // 2 if N > 2 else 1, N))
        if t is not None:
            add("cell_mid_floyd_rejects", f"Floyd draw {t} of the cells rejects once", state_at(b, t, inc, [rejected_value(b[t])]), {t: (once(t), True, None)})
    t = first_rejecting(range(N, 2 * N - 1))
    if t is not None:
        add("cell_fisher_yates_rejects", f"Fisher-Yates draw {t} of the cells rejects once", state_at(b, t, inc, [rejected_value(b[t])]), {t: (once(t), True, None)})
    # a direction draw (bound 4) cannot reject: 0 — leftover 0, rejected under every bound that has a threshold — is taken as it comes
    t = 2 * N - 1
    add("direction_takes_zero", f"direction draw {t} sees 0 and takes it", state_at(b, t, inc, [0]), {t: (0, True, 0)})
    if Q:
        q0 = 3 * N - 1
        t = first_rejecting(range(q0, q0 + Q))
        if t is not None:
            add("queue_first_rejects", f"queue draw {t} rejects", state_at(b, t, inc, [rejected_value(b[t]), rejected_value(b[t], 1)]),
                {t: (AtLeast(1 if takes_high_half(b, t) else 2), True, None)})     # (low half: the high half is rejected too)
        t = first_rejecting(range(len(b) - 1, q0 - 1, -1))
        if t is not None:
            add("queue_last_rejects", f"queue draw {t}, the last one that can, rejects", state_at(b, t, inc, [rejected_value(b[t])]), {t: (once(t), True, None)})
        add("queue_first_value_max", f"queue draw {q0} yields its largest value", state_at(b, q0, inc, [0xFFFFFFFF]), {q0: (0, False, b[q0] - 1)})
    return out


def check_reset_claim(sc, HW, N, S, Q):
    """The tracer's reset from the scenario's state: asserts the claim, returns (cells, dirs, queue, end state words)."""
    t = Tracer(sc.state)
    cells, dirs, queue = t.reset(HW, N, S, Q)
    for i, (redraws, entered, value) in sc.draws.items():
        d = t.draws[i]
        assert redraws_as_claimed(d.redraws, redraws) and d.entered == entered and (value is None or d.value == value), (sc.name, i, d)
    return cells, dirs, queue, t.words()


def shelf_home(highways):
    """(S, 2) (x, y) of shelf id k + 1 after reset: the non-highway cells in row-major order."""
    ys, xs = np.nonzero(np.asarray(highways) == 0)
    return np.stack([xs, ys], 1).astype(np.int32)


# what stands on a delivering goal cell: nobody (the reference pays rewards[-1]), agent 0 carrying the shelf, or another agent
# standing on it without carrying
WHO = ("nobody", "agent_0_carrying", "agent_standing")
DeliveryScenario = namedtuple("DeliveryScenario", "name claim state queue on_goal who draws")   # draws: [(redraws, entered, value or None)]


def delivery_scenarios(S, Q, N, n_goals, inc):
    """One all-NOOP step with requested shelves injected onto goal cells.  `on_goal[g]`: the shelf id on goal g (0: none); the
    replacement draws have the exclusive bound n = S - Q."""
    n = S - Q
    assert n >= 1 and Q >= 1
    out = []
    patterns = {"lowest": list(range(1, Q + 1)), "highest": list(range(S - Q + 1, S + 1))}
    if 2 * Q - 1 <= S:
        patterns["alternating"] = list(range(1, 2 * Q, 2))

    def add(name, claim, state, ids, sids, draws):
        k = len(out)
        queue = ids[k % Q:] + ids[:k % Q]                       # (the delivered id's slot moves through the queue)
        on_goal = [0] * n_goals
        for g, sid in zip(range(n_goals - 1, -1, -1) if k % 2 and len(sids) == 1 else range(n_goals), sids):
            on_goal[g] = sid                                    # (a single delivery alternates between the goals)
        who = WHO[k % 3 if N > 1 else k % 2]
        out.append(DeliveryScenario(name, f"{claim}; {who}", state, queue, on_goal, who, draws))

    idxs = sorted({0, n - 1, n // 4, n // 2, (3 * n) // 4})
    for idx in idxs:
        for pname, ids in patterns.items():
            for which, sid in (("smallest", min(ids)), ("largest", max(ids))):
                state = _state(inc, 0, 0, accepted_value(n, idx), SAFE) if n > 1 else _state(inc, 0, 0, 7, 9)
                add(f"idx_{idx}_{pname}_{which}", f"idx {idx} of {n}, queue of the {pname} ids, the {which} one delivered", state, ids, [sid],
                    [(0, False, idx)])
    ids = patterns.get("alternating", patterns["lowest"])
    if n > 1:
        for c in bounded_cases(n, inc):
            add(f"draw_{c.name}", f"replacement draw: {c.name}", c.state, ids, [ids[len(ids) // 2]], [(c.redraws, c.entered, c.value)])
    c = n1_case(inc)
    if n == 1:
        add("one_candidate_keeps_buffer", "S - Q == 1: nothing consumed, the buffered half stays", c.state, ids, [ids[0]], [(0, False, 0)])
    if n_goals >= 2 and Q >= 2:
        a, b = (n // 3, (2 * n) // 3) if n > 1 else (0, 0)
        va, vb = (accepted_value(n, a), accepted_value(n, b)) if n > 1 else (7, 9)
        two = [ids[0], ids[-1]]
        add("two_goals_fresh_then_buffered", "both goals deliver: the first draw takes the low half, the second the buffered high half",
            _state(inc, 0, 0, va, vb), ids, two, [(0, False, a), (0, False, b)])
        add("two_goals_buffered_then_fresh", "both goals deliver: the first draw takes the buffered half, the second a fresh low half",
            _state(inc, 1, va, vb, SAFE), ids, two, [(0, False, a), (0, False, b)])
        if threshold(n):
            add("two_goals_second_rejects_buffered", "both goals deliver: the second draw rejects the half the first one buffered",
                _state(inc, 0, 0, va, rejected_value(n)), ids, two, [(0, False, a), (1, True, None)])
            add("two_goals_first_rejects_twice", "both goals deliver: the first draw rejects the buffered and the low half",
                _state(inc, 1, rejected_value(n, 1), rejected_value(n), vb), ids, two, [(2, True, b), (0, None, None)])
    return out


def check_delivery_claim(sc, S, Q):
    """Tracer over the scenario's draws; returns (queue after, end state words) by the reference's plain candidate scan."""
    t = Tracer(sc.state)
    queue = list(sc.queue)
    for sid, (redraws, entered, value) in zip([s for s in sc.on_goal if s], sc.draws):
        assert sid in queue, (sc.name, sid, queue)
        idx = t.bounded(S - Q - 1)
        d = t.draws[-1]
        assert (redraws is None or d.redraws == redraws) and (entered is None or d.entered == entered) and (value is None or d.value == value), (sc.name, d)
        cand = [s for s in range(1, S + 1) if s not in queue]
        queue[queue.index(sid)] = cand[idx]
    return queue, t.words()
