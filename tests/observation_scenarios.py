"""Constructed observation states for the step kernels, and a census that names what a state's windows hold.

Random play leaves much of an observation window unseen: a loaded agent facing LEFT in the far corner of the window of the agent
with the highest id, a requested shelf whose id is the last bit of a request word, a window clipped on two sides at once.  This
module BUILDS such states: every window cell with every one of the 15 cell codes (no agent or an agent in one of 4 headings, times
no shelf, an unrequested shelf, a requested shelf), every clip of the window at the borders in every heading, the shelf ids at the
edges of the request words, a full window, every message value at every window cell, and (custom layouts) simultaneous deliveries
on every part of the goal list.

Plain numpy and dicts.  Two entry points:

  build_scenarios(shape, seed)       -> list of scenario dicts: the full injected state of ONE env + 2 steps of actions
                                        (step 0 all NOOP, with message bits where M > 0; step 1 seeded mixed actions)
  window_census(state, shape, msg)   -> Counter of classes of one env's windows, from the state alone (never from an observation)

Only reachable states are built (`check_reachable`): every shelf exists, standing on a non-highway cell or carried on its
carrier's cell, one shelf and one agent per cell, distinct ids in the queue.  Shelves stand on their home cells (shelf id s is the
s-th non-highway cell in row-major order, as reset() leaves them) unless an agent carries them.
"""
from collections import Counter

import numpy as np

UP, DOWN, LEFT, RIGHT = 0, 1, 2, 3
NOOP, FORWARD, TURN_LEFT, TURN_RIGHT, TOGGLE = 0, 1, 2, 3, 4
DXY = {UP: (0, -1), DOWN: (0, 1), LEFT: (-1, 0), RIGHT: (1, 0)}
T_STEPS = 2
FAMILIES = ("code_sweep", "self", "borders", "request_ids", "full_window", "messages", "goals")
ID_ASSIGNMENTS = ("observer_low", "observer_high")
REWARD_TYPES = (0, 1, 2)   # GLOBAL, INDIVIDUAL, TWO_STAGE
NO_AGENT = 2               # a cell code is has_agent | direction one-hot << 1 | has_shelf << 5 | requested << 6 (:655-673)
CODES = tuple(a | s for a in [NO_AGENT] + [1 | (2 << d) for d in range(4)] for s in (0, 32, 96))
REQUEST_IDS = (1, 31, 32, 33, 63, 64, 255, 256, 257)


def make_shape(highways, goals, N, Q, R, M, goals_family=False):
    """`goals_family`: a custom-layout task — its scenarios hold the deliveries, its census the goal classes."""
    hw = np.asarray(highways).astype(bool)
    H, W = hw.shape
    ys, xs = np.nonzero(~hw)
    return dict(H=int(H), W=int(W), hw=hw, goals=[(int(x), int(y)) for x, y in goals], N=int(N), S=int(len(xs)), Q=int(Q), R=int(R),
                M=int(M), home=np.stack([xs, ys], 1).astype(np.int32), goals_family=bool(goals_family))


# ------------------------------------------------------------------------------------------------------------------ census
def check_reachable(st, shape):
    H, W, hw, N, S, Q = (shape[k] for k in ("H", "W", "hw", "N", "S", "Q"))
    cells = [(int(x), int(y)) for x, y in zip(st["agent_x"], st["agent_y"])]
    assert len(set(cells)) == N and all(0 <= x < W and 0 <= y < H for x, y in cells), "one agent per cell, on the grid"
    sxy = [(int(x), int(y)) for x, y in st["shelf_xy"]]
    assert len(sxy) == S and len(set(sxy)) == S, "one shelf per cell"
    carried = {int(c): i for i, c in enumerate(st["agent_carry"]) if c}
    assert len(carried) == sum(1 for c in st["agent_carry"] if c), "a shelf has one carrier"
    for s, c in enumerate(sxy):
        if s + 1 in carried:
            assert c == cells[carried[s + 1]], "a carried shelf is on its carrier's cell"
        else:
            assert not hw[c[1], c[0]], "a standing shelf is on a non-highway cell"
    q = [int(v) for v in st["queue"]]
    assert len(q) == Q and len(set(q)) == Q and all(1 <= v <= S for v in q), "distinct shelf ids in the queue"


def clip_of(x, y, shape):
    R = shape["R"]
    return (max(0, R - x), max(0, x + R - (shape["W"] - 1)), max(0, R - y), max(0, y + R - (shape["H"] - 1)))


def cell_class(c, R):
    """corner / edge (the window's outer ring) / centre_row / inner, of window cell c."""
    WIN = 2 * R + 1
    dx, dy = c % WIN - R, c // WIN - R
    if abs(dx) == R and abs(dy) == R:
        return "corner"
    if dy == 0:
        return "centre_row"
    return "edge" if abs(dx) == R or abs(dy) == R else "inner"


def _layers(st, shape):
    ag = -np.ones((shape["H"], shape["W"]), np.int32)
    sh = np.zeros((shape["H"], shape["W"]), np.int32)
    for i, (x, y) in enumerate(zip(st["agent_x"], st["agent_y"])):
        ag[y, x] = i
    for s, (x, y) in enumerate(st["shelf_xy"]):
        sh[y, x] = s + 1
    return ag, sh


def cell_code(st, shape, i, c, layers=None, queue=None):
    """The 7-bit code observer i sees at window cell c (None when c is off the grid), and the agent / shelf id behind it."""
    R = shape["R"]
    WIN = 2 * R + 1
    x, y = int(st["agent_x"][i]) + c % WIN - R, int(st["agent_y"][i]) + c // WIN - R
    if not (0 <= x < shape["W"] and 0 <= y < shape["H"]):
        return None, -1, 0
    ag, sh = layers or _layers(st, shape)
    j, s = int(ag[y, x]), int(sh[y, x])
    code = (1 | (2 << int(st["agent_dir"][j]))) if j >= 0 else NO_AGENT
    if s:
        code |= 32 | (64 if s in (queue if queue is not None else set(int(q) for q in st["queue"])) else 0)
    return code, j, s


def window_census(st, shape, msg=None):
    """Counter of classes of ONE env: `st` holds agent_x / agent_y / agent_dir / agent_carry (N,), shelf_xy (S, 2), queue (Q,);
    `msg` (N,) the message value every agent shows (the bits of its step-0 action), where M > 0.
      ("cell", c, code)                       per observer and in-grid window cell c other than the centre
      ("clip", left, right, top, bottom)      per observer: window columns / rows that lie off the grid
      ("self", dir, loaded, highway, requested)   per observer
      ("req", word, bit) / ("unreq", word, bit)   per requested / unrequested shelf in a window whose id is bit 0 or 31 of its
                                              request word, or lies in the last word (S >> 5)
      ("lane", j + 1)                         per neighbour j in a window, for the first and the last agent id
      ("msg", value), ("msg_at", cell class, value)   per neighbour in a window
      ("full_window", n)                      per observer with n = min(N - 1, WIN^2 - 1) neighbours in its window: as many as can be
    and, on the custom-layout tasks (shape["goals_family"]) only:
      ("goal", g)                             per agent that stands on goal g of the goal list with a requested shelf on its back
      ("goals_held", k)                       per env with k >= 1 such agents: k deliveries in one step, drawn in goal-list order
    """
    N, S, R, hw = shape["N"], shape["S"], shape["R"], shape["hw"]
    WIN = 2 * R + 1
    out = Counter()
    layers = _layers(st, shape)
    queue = set(int(q) for q in st["queue"])
    for i in range(N):
        x, y = int(st["agent_x"][i]), int(st["agent_y"][i])
        out[("clip",) + clip_of(x, y, shape)] += 1
        carry = int(st["agent_carry"][i])
        out[("self", int(st["agent_dir"][i]), int(carry > 0), int(hw[y, x]), int(carry in queue))] += 1
        crowd = 0
        for c in range(WIN * WIN):
            code, j, s = cell_code(st, shape, i, c, layers, queue)
            if code is None:
                continue
            crowd += int(j >= 0 and j != i)
            if s and ((s & 31) in (0, 31) or (s >> 5) == (S >> 5)):
                out[("req" if s in queue else "unreq", s >> 5, s & 31)] += 1
            if c == WIN * WIN // 2:
                continue
            out[("cell", c, code)] += 1
            if j >= 0:
                if j in (0, N - 1):
                    out[("lane", j + 1)] += 1
                if msg is not None:
                    out[("msg", int(msg[j]))] += 1
                    out[("msg_at", cell_class(c, R), int(msg[j]))] += 1
        if N > 1 and crowd == min(N - 1, WIN * WIN - 1):
            out[("full_window", crowd)] += 1
    held = 0
    for i in range(N if shape["goals_family"] else 0):
        cell = (int(st["agent_x"][i]), int(st["agent_y"][i]))
        if cell in shape["goals"] and int(st["agent_carry"][i]) in queue:
            out[("goal", shape["goals"].index(cell))] += 1
            held += 1
    if held:
        out[("goals_held", held)] += 1
    return out


# --------------------------------------------------------------------------------------------------------------- generator
class _Env:
    """One env under construction: placed agents, carried shelves, ids that must / must not be requested, and the claims
    (observer, window cell, code) every placement made — re-checked after every later placement."""

    def __init__(self, shape):
        self.shape = shape
        self.agents = {}          # id -> [x, y, dir, carry]
        self.req_in, self.req_out = set(), set()
        self.claims = []          # (observer id, window cell, code)
        self.fixed = []           # (agent id, (x, y, dir, carry)): self-family claims

    def copy(self):
        o = _Env(self.shape)
        o.agents = {i: list(a) for i, a in self.agents.items()}
        o.req_in, o.req_out = set(self.req_in), set(self.req_out)
        o.claims, o.fixed = list(self.claims), list(self.fixed)
        return o

    def occupied(self):
        return {(a[0], a[1]) for a in self.agents.values()}

    def carried(self):
        return {a[3] for a in self.agents.values() if a[3]}

    def home_id(self, cell):
        hit = np.nonzero((self.shape["home"] == cell).all(1))[0]
        return int(hit[0]) + 1 if len(hit) else 0

    def place(self, i, cell, d, carry=0):
        """Agent i on `cell`; carry: 0, a shelf id, "home" (the shelf of this non-highway cell) or "spare" (one taken from a far
        cell).  False if that is not a reachable placement."""
        sh = self.shape
        if i in self.agents or cell in self.occupied() or not (0 <= cell[0] < sh["W"] and 0 <= cell[1] < sh["H"]):
            return False
        on_hw = bool(sh["hw"][cell[1], cell[0]])
        if carry == "home":
            carry = self.home_id(cell)
            if not carry:
                return False
        if carry == "spare":
            if not on_hw:
                return False
            taken = self.carried() | self.req_in | self.req_out
            occ = self.occupied()
            far = sorted((s for s in range(1, sh["S"] + 1) if s not in taken and tuple(sh["home"][s - 1]) not in occ),
                         key=lambda s: (-min([abs(sh["home"][s - 1][0] - a[0]) + abs(sh["home"][s - 1][1] - a[1]) for a in self.agents.values()]
                                             + [abs(sh["home"][s - 1][0] - cell[0]) + abs(sh["home"][s - 1][1] - cell[1])]), s))
            if not far:
                return False
            carry = far[0]
        if carry:
            if carry in self.carried():
                return False
            if not on_hw and carry != self.home_id(cell):
                return False      # (a loaded agent stands on a shelf cell only where the shelf it carries is that cell's)
        self.agents[i] = [cell[0], cell[1], d, int(carry)]
        return True

    def request(self, s, wanted):
        (self.req_in if wanted else self.req_out).add(s)
        return not (self.req_in & self.req_out) and len(self.req_in) <= self.shape["Q"] and \
            self.shape["S"] - len(self.req_out) >= self.shape["Q"]

    def state(self, rng=None, fill=True):
        """The scenario's arrays.  Agents not placed yet park on the free cells farthest from the placed ones (`fill`)."""
        sh = self.shape
        N, S, Q = sh["N"], sh["S"], sh["Q"]
        agents = {i: list(a) for i, a in self.agents.items()}
        if fill and len(agents) < N:
            occ = {(a[0], a[1]) for a in agents.values()}
            free = [(x, y) for y in range(sh["H"]) for x in range(sh["W"]) if (x, y) not in occ]
            free.sort(key=lambda c: (-min([abs(c[0] - a[0]) + abs(c[1] - a[1]) for a in agents.values()] or [0]), c[1], c[0]))
            for i in range(N):
                if i not in agents:
                    c = free.pop(0)
                    agents[i] = [c[0], c[1], (i + c[0]) % 4, 0]
        ax, ay, ad, ac = (np.zeros(N, np.int32) for _ in range(4))
        shelf_xy = sh["home"].copy()
        for i, (x, y, d, c) in agents.items():
            ax[i], ay[i], ad[i], ac[i] = x, y, d, c
            if c:
                shelf_xy[c - 1] = (x, y)
        rest = [s for s in range(1, S + 1) if s not in self.req_in and s not in self.req_out]
        if rng is not None:
            rest = [rest[k] for k in rng.permutation(len(rest))]
        queue = sorted(self.req_in) + rest[:Q - len(self.req_in)]
        if rng is not None:
            queue = [queue[k] for k in rng.permutation(len(queue))]
        return dict(agent_x=ax, agent_y=ay, agent_dir=ad, agent_carry=ac, shelf_xy=shelf_xy, queue=np.array(queue, np.int32).reshape(Q))

    def holds(self, fill=True):
        """Every claim made so far still holds in the state as it would be emitted."""
        if len(self.agents) > self.shape["N"]:
            return False
        st = self.state(fill=fill)
        if len(st["queue"]) != self.shape["Q"] or len(set(st["queue"].tolist())) != self.shape["Q"]:
            return False
        layers, queue = _layers(st, self.shape), set(st["queue"].tolist())
        for i, c, code in self.claims:
            if cell_code(st, self.shape, i, c, layers, queue)[0] != code:
                return False
        for i, want in self.fixed:
            if tuple(self.agents[i]) != want:
                return False
        return True


def _cells_from(shape, k):
    """All grid cells, in an order that starts somewhere else for every k (so that items spread over the warehouse)."""
    H, W = shape["H"], shape["W"]
    cells = [(x, y) for y in range(H) for x in range(W)]
    k = (k * 7) % len(cells)
    return cells[k:] + cells[:k]


def _try_item(env, k, obs_id, nb_id, c, code, observer_at=None, observer_dir=None):
    """Observer `obs_id` somewhere (or at `observer_at`) so that its window cell c shows `code`; neighbour `nb_id` where the code
    has an agent.  Returns the new _Env or None."""
    sh = env.shape
    R, hw = sh["R"], sh["hw"]
    WIN = 2 * R + 1
    dx, dy = c % WIN - R, c // WIN - R
    has_agent, shelf = code & 1, (code >> 5) & 3
    d_nb = next((d for d in range(4) if code & (2 << d)), 0) if has_agent else None
    for p in ([observer_at] if observer_at else _cells_from(sh, k)):
        t = (p[0] + dx, p[1] + dy)
        if not (0 <= t[0] < sh["W"] and 0 <= t[1] < sh["H"]) or t == p:
            continue
        t_hw = bool(hw[t[1], t[0]])
        if not shelf and not t_hw:
            continue              # (an empty shelf cell needs a carrier for its shelf: the highway cells give this code)
        if shelf and not has_agent and t_hw:
            continue
        e = env.copy()
        d_obs = (k + p[0] + p[1]) % 4 if observer_dir is None else observer_dir
        if not e.place(obs_id, p, d_obs, 0):
            continue
        sid = 0
        if has_agent:
            carry = 0 if not shelf else "spare" if t_hw else ("home" if k % 2 else 0)
            if not e.place(nb_id, t, d_nb, carry):
                continue
            sid = e.agents[nb_id][3] or (e.home_id(t) if shelf else 0)
        elif shelf:
            sid = e.home_id(t)
            if sid in e.carried():
                continue
        if shelf and not e.request(sid, shelf == 3):
            continue
        e.claims.append((obs_id, c, code))
        if e.holds():
            return e
    return None


class _Packer:
    """Packs items into as few envs as hold them: an item goes into the open env if every claim still holds afterwards."""

    def __init__(self, shape, family, rng, out):
        self.shape, self.family, self.rng, self.out = shape, family, rng, out
        self.env, self.variants, self.assignment = None, [], 0

    def ids(self, n_needed, assignment):
        """The next free agent ids: observers from the low end and neighbours from the high end, or the reverse."""
        used = set(self.env.agents) if self.env else set()
        free = [i for i in range(self.shape["N"]) if i not in used]
        if len(free) < n_needed:
            return None
        lo, hi = free[0], free[-1]
        return (lo, hi) if assignment == 0 else (hi, lo)

    def add(self, variant, assignment, fn, n_agents):
        """fn(env, observer id, neighbour id) -> new env or None."""
        for fresh in (False, True):
            if fresh or self.env is None or assignment != self.assignment:
                self.flush()
                self.env, self.assignment = _Env(self.shape), assignment
            ids = self.ids(n_agents, assignment)
            e = fn(self.env, *ids) if ids else None
            if e is not None:
                self.env = e
                self.variants.append(variant)
                return
        raise AssertionError(f"{self.family}: {variant} cannot be built on this shape")

    def flush(self):
        if self.env is not None and self.variants:
            self.out.append(_emit(self.env, self.family, "+".join(self.variants), self.assignment, self.rng))
        self.env, self.variants = None, []


def _emit(env, family, variant, assignment, rng, actions0=None, reward_type=None, seeded_queue=True):
    sh = env.shape
    N, M = sh["N"], sh["M"]
    st = env.state(rng if seeded_queue else None)
    check_reachable(st, sh)
    actions = np.zeros((T_STEPS, N, 1 + M), np.int32)
    if actions0 is not None:
        actions[0, :, 0] = actions0
    actions[1, :, 0] = rng.choice(5, size=N, p=[0.1, 0.5, 0.1, 0.1, 0.2])
    if M:
        actions[:, :, 1:] = rng.integers(0, 2, size=(T_STEPS, N, M))
    return dict(family=family, variant=variant, ids=assignment, reward_type=reward_type, actions=actions, **st)


def msg_values(actions0):
    """(N,) message value of every agent from its step-0 action row [action, bit 0, bit 1, ...]."""
    bits = np.asarray(actions0)[:, 1:]
    return (bits << np.arange(bits.shape[1])).sum(-1) if bits.shape[1] else None


def _code_sweep(shape, rng, out):
    R = shape["R"]
    WIN = 2 * R + 1
    pk = _Packer(shape, "code_sweep", rng, out)
    k = 0
    for assignment in (0, 1):
        for c in range(WIN * WIN):
            if c == WIN * WIN // 2:
                continue
            for code in CODES:
                k += 1
                pk.add(f"c{c}k{code}", assignment, lambda e, o, n, k=k, c=c, code=code: _try_item(e, k, o, n, c, code), 2 if code & 1 else 1)
    pk.flush()


def _self(shape, rng, out):
    """Every agent id in every (heading, loaded, highway, carried shelf requested) combination."""
    N, hw = shape["N"], shape["hw"]
    combos = [(d, l, h, r) for d in range(4) for l in (0, 1) for h in (0, 1) for r in ((0, 1) if l else (0,))]
    for rot in range(len(combos)):
        env = _Env(shape)
        for i in range(N):
            d, l, h, r = combos[(rot + i * 5) % len(combos)]
            for cell in _cells_from(shape, rot * N + i):
                if bool(hw[cell[1], cell[0]]) != bool(h):
                    continue
                e = env.copy()
                if e.place(i, cell, d, ("spare" if h else "home") if l else 0) and (not l or e.request(e.agents[i][3], bool(r))) and e.holds(fill=False):
                    e.fixed.append((i, tuple(e.agents[i])))
                    env = e
                    break
            else:
                raise AssertionError(("self", rot, i))
        out.append(_emit(env, "self", f"rot{rot}", 0, rng))


def _borders(shape, rng, out):
    """The observer on one cell per distinct clip of its window (all four corners, every distance 0 .. R from every edge), in all 4
    headings; a neighbour on the in-grid window cell next to the clip line(s) — loaded where that is a highway cell, so that
    a shelf stands next to the clip line too."""
    H, W, R = shape["H"], shape["W"], shape["R"]
    WIN = 2 * R + 1
    first = {}
    for y in range(H):
        for x in range(W):
            first.setdefault(clip_of(x, y, shape), (x, y))
    pk = _Packer(shape, "borders", rng, out)
    k = 0
    for clip, p in sorted(first.items()):
        for d in range(4):
            k += 1
            l, r, t, b = clip
            # the in-grid window corner nearest the clipped side(s); an unclipped axis alternates between its two ends
            wx = l if l else (WIN - 1 - r if r else (0 if k % 2 else WIN - 1))
            wy = t if t else (WIN - 1 - b if b else (0 if (k // 2) % 2 else WIN - 1))
            if (wx, wy) == (R, R):   # (sensor range 1 in a corner: that cell is the observer's own; one step along either clip line)
                if k % 2:
                    wx += 1 if l else -1
                else:
                    wy += 1 if t else -1
            c = wy * WIN + wx
            code = (1 | (2 << ((d + k) % 4))) | 32 | (64 if (k // 4) % 2 else 0)
            pk.add(f"clip{l}{r}{t}{b}d{d}", (k // (2 * shape["N"])) % 2, lambda e, o, n, k=k, c=c, code=code, p=p, d=d: _try_item(e, k, o, n, c, code, observer_at=p, observer_dir=d), 2)
    pk.flush()


def _request_ids(shape, rng, out):
    S = shape["S"]
    # the named ids, and every id the census has a class for: bits 0 and 31 of every request word, the whole last word
    ids = sorted({s for s in REQUEST_IDS + (S - 1, S) if 1 <= s <= S} | {s for s in range(1, S + 1) if (s & 31) in (0, 31) or (s >> 5) == (S >> 5)})
    pk = _Packer(shape, "request_ids", rng, out)
    k = 0
    for s in ids:
        home = tuple(int(v) for v in shape["home"][s - 1])
        for carried in (0, 1):
            for wanted in (0, 1):
                k += 1

                def fn(env, o, n, k=k, s=s, carried=carried, wanted=wanted):
                    # the shelf on its home cell (standing, or carried by an agent that picked it up there), or carried on a
                    # neighbouring highway cell; the observer on any free cell that has it in its window
                    R = shape["R"]
                    spots = [home] if not carried else [(home[0] + dx, home[1] + dy) for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1), (0, 0))]
                    for t in spots:
                        if not (0 <= t[0] < shape["W"] and 0 <= t[1] < shape["H"]) or (t != home and not shape["hw"][t[1], t[0]]):
                            continue
                        e0 = env.copy()
                        if s in e0.carried() or (carried and not e0.place(n, t, k % 4, s)) or not e0.request(s, bool(wanted)):
                            continue
                        for p in _cells_from(shape, k):
                            dx, dy = t[0] - p[0], t[1] - p[1]
                            if max(abs(dx), abs(dy)) > R or p == t:
                                continue
                            e = e0.copy()
                            if not e.place(o, p, (k + p[0]) % 4, 0):
                                continue
                            c = (dy + R) * (2 * R + 1) + dx + R
                            e.claims.append((o, c, ((1 | (2 << (k % 4))) if carried else NO_AGENT) | 32 | (64 if wanted else 0)))
                            if e.holds():
                                return e
                    return None
                pk.add(f"id{s}{'c' if carried else 's'}{'r' if wanted else 'u'}", (k // (2 * shape["N"])) % 2, fn, 2 if carried else 1)
    pk.flush()


def _full_window(shape, rng, out):
    """As many of the N agents as the window has cells around one observer, with mixed loads and headings."""
    N, R, H, W, hw = shape["N"], shape["R"], shape["H"], shape["W"], shape["hw"]
    for k, (obs_id, d) in enumerate([(i, d) for i in (0, N - 1) for d in range(4)]):
        p = [(W // 2, H // 2), (1, 1), (W - 2, H - 2), (W // 2 - 1, 1)][k % 4]
        env = _Env(shape)
        assert env.place(obs_id, p, d, 0)
        ring = sorted(((x, y) for y in range(p[1] - R, p[1] + R + 1) for x in range(p[0] - R, p[0] + R + 1)
                       if 0 <= x < W and 0 <= y < H and (x, y) != p), key=lambda c: (max(abs(c[0] - p[0]), abs(c[1] - p[1])), c[1], c[0]))
        others = [i for i in range(N) if i != obs_id]
        if k % 2:
            others.reverse()
        for n, (i, cell) in enumerate(zip(others, ring)):
            load = (n + k) % 3
            carry = 0 if load == 0 else "spare" if hw[cell[1], cell[0]] else "home"
            assert env.place(i, cell, (n + k) % 4, carry), (k, i, cell)
            if carry and (n + k) % 2 and len(env.req_in) < shape["Q"]:
                env.request(env.agents[i][3], True)
        out.append(_emit(env, "full_window", f"obs{obs_id}d{d}", int(obs_id != 0), rng))


def _messages(shape, rng, out):
    """Every message value on a neighbour at every window cell: one (observer, neighbour) pair per env, the other agents parked."""
    N, R, M = shape["N"], shape["R"], shape["M"]
    WIN = 2 * R + 1
    k = 0
    for c in range(WIN * WIN):
        if c == WIN * WIN // 2:
            continue
        for value in range(1 << M):
            k += 1
            a = k % 2
            obs_id, nb_id = (0, N - 1) if a == 0 else (N - 1, 0)
            code = (1 | (2 << (k % 4))) | (32 if k % 3 == 0 else 0)
            env = _try_item(_Env(shape), k, obs_id, nb_id, c, code)
            if env is None:
                env = _try_item(_Env(shape), k, obs_id, nb_id, c, code ^ 32)
            assert env is not None, ("messages", c, value)
            sc = _emit(env, "messages", f"c{c}v{value}", a, rng)
            sc["actions"][0, nb_id, 1:] = [(value >> b) & 1 for b in range(M)]
            out.append(sc)


def _goals(shape, rng, out):
    """k loaded agents, each carrying a requested shelf, step FORWARD onto k distinct goals in the same step — every run of k
    consecutive goals of the goal list, k = 1 .. min(N, Q, n_goals), agent ids ascending and descending along the list (the draw
    order of the replacement requests follows the goal list, not the agent ids), and the first, the middle and the last goal at once
    — and each of these again with the carriers standing on their goals already: they deliver on NOOP.  Every case under GLOBAL,
    INDIVIDUAL and TWO_STAGE rewards."""
    N, Q, H, W, hw, goals = shape["N"], shape["Q"], shape["H"], shape["W"], shape["hw"], shape["goals"]
    G = len(goals)
    cases = []
    for k in range(1, min(N, Q, G) + 1):
        for j in range(G - k + 1):
            for desc in ((0, 1) if k > 1 else (0,)):
                cases.append((f"run{j}k{k}{'d' if desc else 'a'}", list(range(j, j + k)), desc, FORWARD))
    if G > 3:
        cases.append(("spread", [0, G // 2, G - 1][:min(N, Q, 3)], 0, FORWARD))
        cases.append(("spread_d", [0, G // 2, G - 1][:min(N, Q, 3)], 1, FORWARD))
    cases += [("noop_" + name, gis, desc, NOOP) for name, gis, desc, _ in cases]
    for name, gis, desc, act in cases:
        env = _Env(shape)
        acts = np.zeros(N, np.int32)
        chosen = {goals[g] for g in gis}
        ok = True
        for n, g in enumerate(gis):
            i = (N - 1 - n) if desc else n
            gx, gy = goals[g]
            if act == NOOP:
                ok = env.place(i, (gx, gy), n % 4, "spare")
            else:
                ok = False
                # standing on a, heading d, FORWARD lands on the goal; an approach cell that is no goal itself comes first
                approach = sorted(((gx - dx, gy - dy), d) for d, (dx, dy) in DXY.items())
                for a, d in sorted(approach, key=lambda ad: ad[0] in goals):
                    if not (0 <= a[0] < W and 0 <= a[1] < H) or a in chosen or a in env.occupied():
                        continue
                    if env.place(i, a, d, "spare" if hw[a[1], a[0]] else "home"):
                        ok = True
                        break
            if not ok:
                break
            assert env.request(env.agents[i][3], True)
            acts[i] = act
        if not ok:
            continue
        st_rng = np.random.default_rng(int(rng.integers(1 << 30)))
        base = _emit(env, "goals", name, desc, st_rng, actions0=acts)
        for rt in REWARD_TYPES:
            sc = {k2: (v.copy() if isinstance(v, np.ndarray) else v) for k2, v in base.items()}
            sc["reward_type"] = rt
            out.append(sc)


def build_scenarios(shape, seed=0):
    """Scenarios for one task, family by family (shape["goals_family"]: the custom-layout tasks add the deliveries)."""
    rng = np.random.default_rng(seed)
    out = []
    _code_sweep(shape, rng, out)
    _self(shape, rng, out)
    _borders(shape, rng, out)
    _request_ids(shape, rng, out)
    _full_window(shape, rng, out)
    if shape["M"]:
        _messages(shape, rng, out)
    if shape["goals_family"]:
        _goals(shape, rng, out)
    return out


# ------------------------------------------------------------------------------------------------- random play, for the floor
def observer_order_census(st, shape):
    """Counter of ("cell_by", order, c, code) of ONE env — which end of the id range looks at a cell, which decides the lane and so
    the bit alignment of the window rows: for a code with a neighbour in it, order = 0 where the observer's id is below the
    neighbour's, 1 where it is above; for a code without one, 0 for observer id 0 and 1 for observer id N - 1 (others not counted)."""
    N, R = shape["N"], shape["R"]
    WIN = 2 * R + 1
    out = Counter()
    layers, queue = _layers(st, shape), set(int(q) for q in st["queue"])
    for i in range(N):
        for c in range(WIN * WIN):
            code, j, _ = cell_code(st, shape, i, c, layers, queue)
            if code is None or c == WIN * WIN // 2:
                continue
            if j >= 0:
                out[("cell_by", int(i > j), c, code)] += 1
            elif i in (0, N - 1):
                out[("cell_by", int(i == N - 1 and N > 1), c, code)] += 1
    return out


def census_key(cls):
    return "/".join(str(v) for v in cls)


def random_play_classes(orc, shape, steps, seed=5):
    """The census classes that `steps` steps of random play reach on an OracleVecEnv (actions p = [.05, .7, .1, .1, .05], random
    message bits), counted on the states the oracle holds — reset states included."""
    rng = np.random.default_rng(3)
    N, M = shape["N"], shape["M"]
    orc.reset(seed=seed)
    seen = Counter()
    for t in range(steps):
        a = np.zeros((orc.B, N, 1 + M), np.int32)
        a[:, :, 0] = rng.choice(5, size=(orc.B, N), p=[.05, .7, .1, .1, .05])
        if M:
            a[:, :, 1:] = rng.integers(0, 2, size=(orc.B, N, M))
        orc.step_autoreset(a, "next_step")
        st, sxy = orc.get_state(), orc.shelf_xy()
        for e in range(orc.B):
            one = dict(agent_x=st["agent_x"][e], agent_y=st["agent_y"][e], agent_dir=st["agent_dir"][e], agent_carry=st["agent_carry"][e],
                       shelf_xy=sxy[e], queue=st["queue"][e])
            seen.update(window_census(one, shape, st["agent_msg"][e] if M else None))
    return seen
