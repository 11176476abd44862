"""Constructed states for what a step does AFTER the moves are committed (rware/warehouse.py:889-941) — TOGGLE_LOAD, the goal loop,
request replacement, the three reward types, the two counters and the termination test — and a census that names what one step of one
env held.

The step kernels keep this phase in several hand-kept texts: the load / unload block three times (register, per-cell LDS and wide agent
phases), counters and termination twice (`goals_and_termination`, and a register shortcut that the exact-shape builds take whenever a
prefilter built from registers and cross-lane votes decides that nothing can be delivered).  A wrong prefilter does not deliver wrongly:
it does not deliver at all.  Random and scripted play reach few of the states that tell those texts apart, so this module BUILDS them.

Plain numpy; the engine is not imported.  Two entry points:

  handling_census(before, actions, after, deliveries, shape) -> Counter of classes of ONE step of ONE env (any trace, not only built ones)
  build_scenarios(shape, seed)                               -> list of scenario dicts: the injected state of one env + T_STEPS x N actions

A state is a dict of agent_x / agent_y / agent_dir / agent_carry / agent_delivered (N,), queue (Q,), steps, inactive and the shelves as
`shelf_xy` (S, 2) or `shelf_layer` (H, W; carried shelves under their carriers, as `_recalc_grid` leaves them).  `shape` holds H, W, N,
S, Q, goals [(x, y)] in the reference's order, highways (H, W), reward_type (0 GLOBAL, 1 INDIVIDUAL, 2 TWO_STAGE), max_steps and
max_inactivity_steps (None or 0: no limit); build_scenarios also reads shelf_xy (every shelf's home), queue and rng0 of a seeded reset.

Every scenario runs under the four CONFIGS — the three reward types with both limits set to LIMITS, and TWO_STAGE with no limit at all
— so a claim names classes that hold under every reward type (`a|b`: either), at step 0 or at `@t`; `L:` / `U:` parts are read only
with / without limits.
"""
from collections import Counter

import numpy as np

import rng_states as rs

UP, DOWN, LEFT, RIGHT = 0, 1, 2, 3
NOOP, FORWARD, TURN_LEFT, TURN_RIGHT, TOGGLE = 0, 1, 2, 3, 4
DXY = {UP: (0, -1), DOWN: (0, 1), LEFT: (-1, 0), RIGHT: (1, 0)}
OPP = {UP: DOWN, DOWN: UP, LEFT: RIGHT, RIGHT: LEFT}
_TURN_L = {UP: LEFT, LEFT: DOWN, DOWN: RIGHT, RIGHT: UP}
_TURN_R = {v: k for k, v in _TURN_L.items()}
T_STEPS = 6
GLOBAL, INDIVIDUAL, TWO_STAGE = 0, 1, 2
LIMITS = dict(max_steps=12, max_inactivity_steps=9)     # small enough to inject counters next to, large enough that no other scenario ends
CONFIGS = ((GLOBAL, True), (INDIVIDUAL, True), (TWO_STAGE, True), (TWO_STAGE, False))   # (reward type, limits set)
NEAR_2_30 = (1 << 30) - 8                                # a counter from here on counts as "near 2^30"

FAMILIES = ("pickup", "unload", "delivery", "chain", "goal_moves", "toggle_vs_mover", "payments", "limits", "story")
ID_ASSIGNMENTS = ("lowest", "highest", "b5_6", "b11_12", "b12_13", "b15_16", "b63_64")
HANDLED_IDS = (1, 31, 32, 33, 63, 64, 255, 256, 257)    # and S - 1, S: both sides of every word of the requested-shelf bitmap
EDGE_TAGS = ("_bit0", "_bit31", "_word_first", "_word_last")


def config_shape(shape, c):
    """`shape` under configuration c of CONFIGS."""
    rt, limited = CONFIGS[c]
    out = dict(shape, reward_type=rt)
    out.update(LIMITS if limited else dict(max_steps=None, max_inactivity_steps=None))
    return out


PER_CONFIG = ("r_agent_delivered", "r_rewards_x2", "r_done", "r_steps", "r_inactive")   # what the generator records per configuration


def config_view(z, c):
    """A recorded fixture (tests/golden/handling) under configuration c in the form tests/pins.py replays — r_<field>[scenario, step]:
    the PER_CONFIG arrays are recorded as [scenario, configuration, step, ...]; `config` says which one this is."""
    return dict({k: (a[:, c] if k in PER_CONFIG else a) for k, a in z.items()}, config=c)


# ------------------------------------------------------------------------------------------------------------------ census
def _layer(state, H, W):
    if "shelf_layer" in state:
        return np.asarray(state["shelf_layer"])
    xy = np.asarray(state["shelf_xy"])
    layer = np.zeros((H, W), np.int32)
    layer[xy[:, 1], xy[:, 0]] = np.arange(1, len(xy) + 1)
    return layer


def edge_tags(cell, H, W):
    """Where the cell's bit lies in the per-cell bitmaps the kernels keep (highways: one bit per cell, 32 to a word)."""
    idx = cell[1] * W + cell[0]
    return [t for t, hit in zip(EDGE_TAGS, (idx & 31 == 0, idx & 31 == 31, idx >> 5 == 0, idx >> 5 == (H * W - 1) >> 5)) if hit]


def paid_unloads(before, actions, shape):
    """Agents whose unload pays the second stage this step (:893-897)."""
    hw = np.asarray(shape["highways"])
    return [i for i in range(shape["N"]) if int(actions[i]) == TOGGLE and before["agent_carry"][i] and before["agent_delivered"][i]
            and not hw[before["agent_y"][i], before["agent_x"][i]] and shape["reward_type"] == TWO_STAGE]


def count_deliveries(before, actions, rewards, shape):
    """The step's delivery count from its rewards (a trace holds no draw count): every delivery pays 1 to everybody (GLOBAL), 1 to
    one agent (INDIVIDUAL) or 0.5 to one agent beside the 0.5 of every paid unload (TWO_STAGE)."""
    r = np.asarray(rewards, np.float64)
    if shape["reward_type"] == GLOBAL:
        return int(round(r[0]))
    if shape["reward_type"] == INDIVIDUAL:
        return int(round(r.sum()))
    return int(round(2 * r.sum())) - len(paid_unloads(before, actions, shape))


def handling_census(before, actions, after, deliveries, shape):
    """Counter of the classes ONE step of ONE env holds.  `deliveries`: the step's replacement draws (ref_step_events; a changed queue
    slot is not a count — a chained delivery writes one slot twice); None: taken as the goals whose shelf the start-of-step queue holds.

      pick / pick_on_highway / pick_on_goal / pick_nothing      per unloaded agent that sends TOGGLE_LOAD: a shelf stands under it (on a
                                                                highway / goal cell, where only an injected state has one) or not
      drop / drop_paid / drop_flag_cleared_unpaid               per loaded agent that sends it off the highways: `has_delivered` set and
                                                                the reward type TWO_STAGE / set and another type
      drop_refused_on_highway                                   ... on a highway cell: nothing happens, the flag stays
          (the latter two also with _bit0 / _bit31 / _word_first / _word_last: where the cell lies in the highway bitmap)
      delivery_by_arrival_g<k> / delivery_in_place              per delivering goal k: its carrier moved onto it this step / did not move
      delivery_nobody_on_goal                                   ... no agent stands there: the reference pays rewards[-1]
      delivery_standing_under_unloaded_agent                    ... the agent that stands there does not carry the shelf
      two_deliveries                                            the step delivered twice or more
      chained_delivery                                          per goal that delivered a shelf the start-of-step queue did not hold: an
                                                                earlier goal's replacement draw requested it (one slot written twice)
      reverse_chain                                             per goal that holds, after the step, a shelf which a LATER goal's draw has
                                                                just requested: it delivers on the next step, in place
      goal_to_goal_loaded / loaded_leaves_goal                  per loaded mover from a goal cell to a goal cell / to another cell
      arrives_as_other_leaves                                   per mover onto a goal cell another mover left, one of them loaded
      follow_across_goals                                       ... that itself came from a goal cell
      swap_on_goals                                             per refused 2-swap on two goal cells
      unloaded_leaves_standing_requested                        per unloaded mover off a goal cell on which a requested shelf stands
      both_payments_one_slot                                    the LAST agent unloads with the flag set while a goal nobody stands on pays
                                                                rewards[-1]: under TWO_STAGE 1.0 in one slot, and the flag ends set
      max_steps_* / max_inactivity_steps_*                      due_with_delivery, due_without_delivery (inactivity: would be due, the
                                                                delivery resets it), one_before, none_counter_near_2_30; both_limits_due
    """
    H, W, N = int(shape["H"]), int(shape["W"]), int(shape["N"])
    goals = [tuple(int(v) for v in g) for g in shape["goals"]]
    goalset = set(goals)
    hw = np.asarray(shape["highways"])
    rt = int(shape["reward_type"])
    L0, L1 = _layer(before, H, W), _layer(after, H, W)
    lst = lambda a: np.asarray(a).tolist()  # noqa: E731
    pos0, pos1 = list(zip(lst(before["agent_x"]), lst(before["agent_y"]))), list(zip(lst(after["agent_x"]), lst(after["agent_y"])))
    carry0, flag0, carry1, dir0 = lst(before["agent_carry"]), lst(before["agent_delivered"]), lst(after["agent_carry"]), lst(before["agent_dir"])
    moved = [a != b for a, b in zip(pos0, pos1)]
    q0, q1 = lst(before["queue"]), lst(after["queue"])
    actions = lst(actions)
    out = Counter()

    # ---- TOGGLE_LOAD (:889-899)
    for i in range(N):
        if actions[i] != TOGGLE:
            continue
        c = pos0[i]
        if not carry0[i]:
            if L0[c[1], c[0]]:
                out["pick"] += 1
                out["pick_on_highway"] += int(bool(hw[c[1], c[0]]))
                out["pick_on_goal"] += int(c in goalset)
            else:
                out["pick_nothing"] += 1
            continue
        if hw[c[1], c[0]]:
            cls = "drop_refused_on_highway"
        else:
            out["drop"] += 1
            cls = ("drop_paid" if rt == TWO_STAGE else "drop_flag_cleared_unpaid") if flag0[i] else None
        if cls:
            out[cls] += 1
            if cls != "drop_paid":
                for tag in edge_tags(c, H, W):
                    out[cls + tag] += 1

    # ---- the goal loop (:903-927): which goals delivered
    direct, q = [], list(q0)
    for k, g in enumerate(goals):
        sid = int(L1[g[1], g[0]])
        if sid and sid in q:
            q[q.index(sid)] = -1
            direct.append(k)
    D = len(direct) if deliveries is None else int(deliveries)
    chained = []
    if D > len(direct):     # the rest delivered a shelf that an earlier delivery of this step requested
        for k, g in enumerate(goals):
            sid = int(L1[g[1], g[0]])
            if len(chained) < D - len(direct) and sid and k not in direct and sid not in q0 and sid not in q1 and any(d < k for d in direct + chained):
                chained.append(k)
    assert D == len(direct) + len(chained), f"{D} deliveries, but the goals explain {direct} + {chained}"
    at1 = {p: i for i, p in enumerate(pos1)}
    nobody = False
    for k in sorted(direct + chained):
        g = goals[k]
        sid, i = int(L1[g[1], g[0]]), at1.get(g)
        if i is None:
            out["delivery_nobody_on_goal"] += 1
            nobody = True
        elif carry1[i] != sid:
            out["delivery_standing_under_unloaded_agent"] += 1
        elif moved[i]:
            out[f"delivery_by_arrival_g{k}"] += 1
        else:
            out["delivery_in_place"] += 1
    out["two_deliveries"] += int(D >= 2)
    out["chained_delivery"] += len(chained)
    for k, g in enumerate(goals):
        sid = int(L1[g[1], g[0]])
        if sid and sid in q1 and sid not in q0 and k not in direct + chained and any(d > k for d in direct + chained):
            out["reverse_chain"] += 1

    # ---- moves on and off the goal cells
    left = {pos0[i]: i for i in range(N) if moved[i] and pos0[i] in goalset}
    for i in range(N):
        if not moved[i]:
            continue
        a, b = pos0[i], pos1[i]
        if a in goalset and carry0[i]:
            out["goal_to_goal_loaded" if b in goalset else "loaded_leaves_goal"] += 1
        if b in left and (carry0[i] or carry0[left[b]]):
            out["arrives_as_other_leaves"] += 1
            out["follow_across_goals"] += int(a in goalset)
        if a in goalset and not carry0[i] and int(L0[a[1], a[0]]) in q0:
            out["unloaded_leaves_standing_requested"] += 1

    def target(i):
        dx, dy = DXY[dir0[i]]
        return (pos0[i][0] + dx, pos0[i][1] + dy) if actions[i] == FORWARD else pos0[i]

    on_goal = [i for i in range(N) if pos0[i] in goalset and actions[i] == FORWARD]
    out["swap_on_goals"] += sum(1 for i in on_goal for j in on_goal if i < j and target(i) == pos0[j] and target(j) == pos0[i])

    last = N - 1
    if actions[last] == TOGGLE and carry0[last] and flag0[last] and not hw[pos0[last][1], pos0[last][0]] and nobody:
        out["both_payments_one_slot"] += 1

    # ---- counters and termination (:929-941)
    ms, mi = shape.get("max_steps") or 0, shape.get("max_inactivity_steps") or 0
    s0, i0 = int(before["steps"]), int(before["inactive"])
    how = "with_delivery" if D else "without_delivery"
    s_due, i_due = bool(ms) and s0 + 1 >= ms, bool(mi) and i0 + 1 >= mi
    out[f"max_steps_due_{how}"] += int(s_due)
    out[f"max_inactivity_steps_due_{how}"] += int(i_due)
    out["both_limits_due"] += int(s_due and i_due)
    out["max_steps_one_before"] += int(bool(ms) and s0 + 2 == ms)
    out["max_inactivity_steps_one_before"] += int(bool(mi) and i0 + 2 == mi and not D)
    out["max_steps_none_counter_near_2_30"] += int(not ms and s0 >= NEAR_2_30)
    out["max_inactivity_steps_none_counter_near_2_30"] += int(not mi and i0 >= NEAR_2_30)
    return +out


def claim_holds(by_step, claim, limited):
    """`by_step`: the census of every step of one scenario under one configuration.  `claim`: parts joined by '+'; a part is
    [L: | U:] class [| class ...] [@step] — any of the classes, at that step (0 if not said); L: / U: parts count only under a
    configuration with / without limits."""
    for part in claim.split("+"):
        if part[:2] in ("L:", "U:"):
            if (part[0] == "L") != limited:
                continue
            part = part[2:]
        part, _, t = part.partition("@")
        if not any(by_step[int(t or 0)].get(c, 0) for c in part.split("|")):
            return False
    return True


def admitted(shape):
    """(families, classes) that the geometry and the agent count of `shape` admit; the classes over all four CONFIGS."""
    g = _Geo(shape)
    N, H, W = g.N, g.H, g.W
    fam = {"pickup", "unload", "delivery", "payments", "limits"}
    cls = {"pick", "pick_on_highway", "pick_on_goal", "pick_nothing", "drop", "drop_paid", "drop_flag_cleared_unpaid", "drop_refused_on_highway",
           "delivery_in_place", "delivery_nobody_on_goal", "delivery_standing_under_unloaded_agent", "unloaded_leaves_standing_requested",
           "loaded_leaves_goal", "both_payments_one_slot", "both_limits_due", "max_steps_one_before", "max_inactivity_steps_one_before",
           "max_steps_none_counter_near_2_30", "max_inactivity_steps_none_counter_near_2_30"}
    cls |= {f"{lim}_due_{how}" for lim in ("max_steps", "max_inactivity_steps") for how in ("with_delivery", "without_delivery")}
    cls |= {f"delivery_by_arrival_g{k}" for k, gc in enumerate(g.goals) if g.approaches(gc)}
    for y in range(H):
        for x in range(W):
            if (x, y) not in g.goalset:
                base = "drop_refused_on_highway" if g.hw[y, x] else "drop_flag_cleared_unpaid"
                cls |= {base + t for t in edge_tags((x, y), H, W)}
    if len(g.goals) >= 2 and g.Q >= 2:
        cls.add("two_deliveries")
    if len(g.goals) >= 2 and g.S - g.Q >= 2:
        fam.add("chain")
        cls |= {"chained_delivery", "two_deliveries", "reverse_chain"}
    if g.adjacent:
        fam.add("goal_moves")
        cls.add("goal_to_goal_loaded")
        if N >= 2:
            cls |= {"arrives_as_other_leaves", "follow_across_goals", "swap_on_goals"}
    if N >= 2 and g.mover_spots():
        fam.add("toggle_vs_mover")
    if g.story_spots():
        fam.add("story")
    return fam, cls


# ------------------------------------------------------------------------------------------------------------------ geometry
class _Geo:
    def __init__(self, shape):
        self.H, self.W, self.N = int(shape["H"]), int(shape["W"]), int(shape["N"])
        self.hw = np.asarray(shape["highways"])
        self.goals = [tuple(int(v) for v in g) for g in shape["goals"]]
        self.goalset = set(self.goals)
        self.S = int(shape["S"]) if "S" in shape else int((self.hw == 0).sum())
        self.Q = int(shape["Q"])
        homes = rs.shelf_home(self.hw)
        self.home = {s + 1: (int(x), int(y)) for s, (x, y) in enumerate(homes)}
        self.home_at = {c: s for s, c in self.home.items()}
        self.adjacent = [(a, b) for a in range(len(self.goals)) for b in range(len(self.goals))
                         if a != b and abs(self.goals[a][0] - self.goals[b][0]) + abs(self.goals[a][1] - self.goals[b][1]) == 1]

    def inb(self, c):
        return 0 <= c[0] < self.W and 0 <= c[1] < self.H

    def step(self, c, d, k=1):
        return (c[0] + DXY[d][0] * k, c[1] + DXY[d][1] * k)

    def approaches(self, g):
        """[(cell, direction from it onto g)]: the neighbours of goal cell g that are highway cells and no goal cells."""
        out = []
        for d in (LEFT, RIGHT, UP, DOWN):
            c = self.step(g, d)
            if self.inb(c) and c not in self.goalset and self.hw[c[1], c[0]]:
                out.append((c, OPP[d]))
        return out

    def highway_cells(self):
        return [(x, y) for y in range(self.H) for x in range(self.W) if self.hw[y, x] and (x, y) not in self.goalset]

    def mover_spots(self):
        """[(shelf cell c, highway cell m next to it, direction m -> c)]: where a loaded mover can face an occupied shelf cell."""
        out = []
        for sid, c in self.home.items():
            for d in (LEFT, RIGHT, UP, DOWN):
                m = self.step(c, d)
                if self.inb(m) and self.hw[m[1], m[0]] and m not in self.goalset and not any(abs(m[0] - g[0]) + abs(m[1] - g[1]) <= 1 for g in self.goals):
                    out.append((c, m, OPP[d]))
        return out

    def story_spots(self):
        """[(goal index, approach cell, direction, shelf cell straight behind the goal)]: deliver, carry off and unload in three steps."""
        out = []
        for k, g in enumerate(self.goals):
            for a, d in self.approaches(g):
                h = self.step(g, d)
                if self.inb(h) and not self.hw[h[1], h[0]]:
                    out.append((k, a, d, h))
        return out


# --------------------------------------------------------------------------------------------------------------- generator
class _Actor:
    def __init__(self, cell, d, acts, carry=0, flag=0):
        self.cell, self.dir, self.acts, self.carry, self.flag = cell, d, list(acts) + [NOOP] * (T_STEPS - len(acts)), carry, flag


class _Proto:
    """One situation before agent ids are assigned.  `place`: standing shelves {id: cell}; `requested` / `unrequested`: what the queue
    must / must not hold; `draws`: [(delivered id, id its replacement draw must return)] of step 0, in goal order; `pin_last`: index of
    the actor that must be the last agent."""

    def __init__(self, family, variant, claim, actors=(), place=None, requested=(), unrequested=(), draws=(), steps=0, inactive=0, pin_last=None):
        self.family, self.variant, self.claim, self.actors = family, variant, claim, list(actors)
        self.place, self.requested, self.unrequested, self.draws = dict(place or {}), list(requested), list(unrequested), list(draws)
        self.steps, self.inactive, self.pin_last = steps, inactive, pin_last


def _protos(g, shape):
    P = []
    S, Q, N = g.S, g.Q, g.N
    handled = [s for s in dict.fromkeys(HANDLED_IDS[:6] + (S - 1, S) + HANDLED_IDS[6:]) if 1 <= s <= S]
    rot = [0]

    def sid_next(avoid=()):
        for _ in range(len(handled) + 1):
            s = handled[rot[0] % len(handled)]
            rot[0] += 1
            if s not in avoid:
                return s
        return next(s for s in range(S, 0, -1) if s not in avoid)

    hcells = g.highway_cells()
    # highway cells off the left wall, the farthest from every goal first: where a lone agent toggles undisturbed
    quiet = sorted((c for c in hcells if c[0] != 0), key=lambda c: (-min(abs(c[0] - q[0]) + abs(c[1] - q[1]) for q in g.goals), c[1], c[0]))[:4]
    assert len(quiet) >= 3 and all(min(abs(c[0] - q[0]) + abs(c[1] - q[1]) for q in g.goals) >= 2 for c in quiet)
    edge_hw = [c for c in hcells if edge_tags(c, g.H, g.W) and c[0] != 0]
    edge_hw = list({tuple(edge_tags(c, g.H, g.W)): c for c in edge_hw}.values())
    shelf_cells = sorted(g.home_at, key=lambda c: (c[1], c[0]))
    edge_sh = list({tuple(edge_tags(c, g.H, g.W)): c for c in shelf_cells if edge_tags(c, g.H, g.W)}.values())
    paid = "drop_paid|drop_flag_cleared_unpaid"
    some_goals = sorted({0, min(1, len(g.goals) - 1), len(g.goals) - 1})

    # ---- 1. pick-ups
    for n, s in enumerate(handled):
        flag = n % 2     # (an unloaded agent with the flag set: it stood on a delivering goal without carrying)
        P.append(_Proto("pickup", f"home_{s}_flag{flag}", "pick+drop@1+pick@2" + (f"+{paid}@1" if flag else ""),
                        [_Actor(g.home[s], UP, [TOGGLE, TOGGLE, TOGGLE], 0, flag)], unrequested=[s] if n % 3 else [], requested=[] if n % 3 else [s]))
    for n, c in enumerate(edge_hw + quiet[:2]):
        s = sid_next()
        tags = "".join(f"+drop_refused_on_highway{t}@1" for t in edge_tags(c, g.H, g.W))
        P.append(_Proto("pickup", f"highway_{c[0]}_{c[1]}_shelf_{s}", "pick+pick_on_highway+drop_refused_on_highway@1" + tags,
                        [_Actor(c, DOWN, [TOGGLE, TOGGLE, TURN_LEFT, TOGGLE], 0, n % 2)], place={s: c}, unrequested=[s]))
    for k in some_goals:
        for req in (False, True):
            s = sid_next()
            P.append(_Proto("pickup", f"goal{k}_shelf_{s}_{'requested' if req else 'unrequested'}", "pick+pick_on_goal" + ("+delivery_in_place" if req else ""),
                            [_Actor(g.goals[k], UP, [TOGGLE, TOGGLE, NOOP, TOGGLE])], place={s: g.goals[k]}, requested=[s] if req else [], unrequested=[] if req else [s]))
    P.append(_Proto("pickup", "nothing_on_highway", "pick_nothing", [_Actor(quiet[0], UP, [TOGGLE, TOGGLE])]))
    s = sid_next()
    P.append(_Proto("pickup", f"nothing_on_emptied_home_{s}", "pick_nothing", [_Actor(g.home[s], LEFT, [TOGGLE, NOOP, TOGGLE])], place={s: quiet[1]}, unrequested=[s]))

    # ---- 2. unloads
    for n, s in enumerate(handled):
        flag = (n + 1) % 2
        P.append(_Proto("unload", f"home_{s}_flag{flag}", "drop+pick@1+drop@2" + (f"+{paid}" if flag else ""),
                        [_Actor(g.home[s], RIGHT, [TOGGLE, TOGGLE, TOGGLE], s, flag)], unrequested=[s] if n % 2 else [], requested=[] if n % 2 else [s]))
    for c in edge_sh:
        s = g.home_at[c]
        tags = "".join(f"+drop_paid|drop_flag_cleared_unpaid{t}" for t in edge_tags(c, g.H, g.W))
        P.append(_Proto("unload", f"edge_{c[0]}_{c[1]}_shelf_{s}", f"drop+{paid}" + tags, [_Actor(c, DOWN, [TOGGLE, NOOP, TOGGLE, TOGGLE], s, 1)], unrequested=[s]))
    for n, c in enumerate(edge_hw + quiet[:2]):
        s = sid_next()
        tags = "".join(f"+drop_refused_on_highway{t}" for t in edge_tags(c, g.H, g.W))
        P.append(_Proto("unload", f"refused_{c[0]}_{c[1]}_shelf_{s}_flag{n % 2}", "drop_refused_on_highway" + tags,
                        [_Actor(c, UP, [TOGGLE, TOGGLE, TURN_RIGHT, TOGGLE], s, n % 2)], unrequested=[s]))
    for k in some_goals:
        for req in (False, True):
            s = sid_next()
            P.append(_Proto("unload", f"refused_goal{k}_shelf_{s}_{'requested' if req else 'unrequested'}", "drop_refused_on_highway" + ("+delivery_in_place" if req else ""),
                            [_Actor(g.goals[k], UP, [TOGGLE, TOGGLE], s, int(not req))], requested=[s] if req else [], unrequested=[] if req else [s]))

    # ---- 3. deliveries.  kinds of what stands on a goal: a = arrives loaded, i = loaded in place, n = nobody (standing shelf),
    #         u = an unloaded agent stands on the standing shelf, w = an unloaded agent walks onto it
    def on_goal(k, kind, s, which=0, then=()):
        """(actors, place) that put shelf s onto goal k in the given way."""
        gc = g.goals[k]
        ap = g.approaches(gc)
        if kind in "aw" and not ap:
            return None
        if kind in "aw":
            c, d = ap[which % len(ap)]
            if kind == "a":
                return [_Actor(c, d, [FORWARD] + list(then), s)], {}
            return [_Actor(c, d, [FORWARD] + list(then))], {s: gc}
        if kind == "i":
            return [_Actor(gc, UP, [NOOP] + list(then), s)], {}
        if kind == "u":
            return [_Actor(gc, DOWN, [NOOP] + list(then))], {s: gc}
        return [], {s: gc}

    names = dict(a=lambda k: f"delivery_by_arrival_g{k}", i=lambda k: "delivery_in_place", n=lambda k: "delivery_nobody_on_goal",
                 u=lambda k: "delivery_standing_under_unloaded_agent", w=lambda k: "delivery_standing_under_unloaded_agent")
    for k in range(len(g.goals)):
        for kind in "ainuw":
            for which in range(len(g.approaches(g.goals[k])) if kind == "a" else 1):
                s = sid_next()
                then = [TURN_LEFT, TURN_LEFT, FORWARD] if kind == "a" else [NOOP, NOOP, TOGGLE] if kind == "i" else []
                got = on_goal(k, kind, s, which, then)
                if got is None:
                    continue
                new = sid_next(avoid=[s])
                P.append(_Proto("delivery", f"g{k}_{kind}{which}_shelf_{s}_then_{new}", names[kind](k) + ("+loaded_leaves_goal@3" if kind == "a" else ""),
                                got[0], got[1], requested=[s], unrequested=[new], draws=[(s, new)]))
        s = sid_next()
        ap = g.approaches(g.goals[k])
        if ap:      # an unloaded agent walks off a goal on which a requested shelf stands
            P.append(_Proto("delivery", f"g{k}_unloaded_leaves_shelf_{s}", "unloaded_leaves_standing_requested+delivery_nobody_on_goal",
                            [_Actor(g.goals[k], OPP[ap[0][1]], [FORWARD])], {s: g.goals[k]}, requested=[s]))
    pairs = [(0, 1)] + ([(len(g.goals) - 1, len(g.goals) - 2), (1, len(g.goals) - 1)] if len(g.goals) > 2 else []) if len(g.goals) >= 2 else []
    if Q >= 2:
        for ka, kb in pairs:
            for kinds in ("aa", "ia", "ni", "an", "nn", "ui", "wa"):
                s1, s2 = sid_next(), 0
                s2 = sid_next(avoid=[s1])
                A, B = on_goal(ka, kinds[0], s1), on_goal(kb, kinds[1], s2, 1)
                if A is None or B is None:
                    continue
                n1 = sid_next(avoid=[s1, s2])
                n2 = sid_next(avoid=[s1, s2, n1])
                first = [(s1, n1), (s2, n2)] if ka < kb else [(s2, n2), (s1, n1)]
                P.append(_Proto("delivery", f"two_g{ka}{kinds[0]}_g{kb}{kinds[1]}_shelves_{s1}_{s2}", f"two_deliveries+{names[kinds[0]](ka)}+{names[kinds[1]](kb)}",
                                A[0] + B[0], {**A[1], **B[1]}, requested=[s1, s2], unrequested=[n1, n2], draws=first))

    # ---- 4. chained deliveries: goal k delivers a, its draw requests b, which stands on a later goal (delivers at once, the slot is
    #         written twice) or on an earlier one (delivers on the next step, in place)
    if len(g.goals) >= 2 and S - Q >= 2:
        for ka, kb in [(0, 1)] + ([(len(g.goals) - 2, len(g.goals) - 1), (0, len(g.goals) - 1)] if len(g.goals) > 2 else []):
            for kinds in ("nn", "ii", "ai", "na", "in", "iu"):
                if len(kinds.replace("n", "")) > N:
                    continue
                a, b = sid_next(), 0
                b = sid_next(avoid=[a])
                c = sid_next(avoid=[a, b])
                A, B = on_goal(ka, kinds[0], a), on_goal(kb, kinds[1], b, 1)
                if A is not None and B is not None:
                    P.append(_Proto("chain", f"chained_g{ka}{kinds[0]}_g{kb}{kinds[1]}_shelves_{a}_{b}_{c}", "chained_delivery+two_deliveries",
                                    A[0] + B[0], {**A[1], **B[1]}, requested=[a], unrequested=[b, c], draws=[(a, b), (b, c)]))
                A, B = on_goal(kb, kinds[0], a), on_goal(ka, kinds[1], b, 1)
                if A is not None and B is not None and kinds[1] != "w":
                    nxt = "delivery_in_place|delivery_nobody_on_goal|delivery_standing_under_unloaded_agent@1"
                    P.append(_Proto("chain", f"reverse_g{kb}{kinds[0]}_g{ka}{kinds[1]}_shelves_{a}_{b}", "reverse_chain+" + nxt,
                                    A[0] + B[0], {**A[1], **B[1]}, requested=[a], unrequested=[b], draws=[(a, b)]))

    # ---- 5. moves between and off adjacent goal cells
    for ka, kb in g.adjacent:
        ga, gb = g.goals[ka], g.goals[kb]
        d_ab = next(d for d in DXY if g.step(ga, d) == gb)
        outs_a = [(c, OPP[d]) for c, d in g.approaches(ga)]      # (cell next to ga, direction from ga to it)
        outs_b = [(c, OPP[d]) for c, d in g.approaches(gb)]
        for req in (True, False):
            s = sid_next()
            P.append(_Proto("goal_moves", f"g{ka}_to_g{kb}_shelf_{s}_{'requested' if req else 'unrequested'}",
                            "goal_to_goal_loaded" + (f"+delivery_by_arrival_g{kb}" if req else ""), [_Actor(ga, d_ab, [FORWARD, FORWARD], s)],
                            requested=[s] if req else [], unrequested=[] if req else [s]))
        for c, d in outs_a[:2]:
            s = sid_next()
            P.append(_Proto("goal_moves", f"g{ka}_leaves_loaded_{d}_shelf_{s}", "loaded_leaves_goal", [_Actor(ga, d, [FORWARD, TURN_LEFT], s)], requested=[s]))
        if N < 2:
            continue
        # A leaves ga, B arrives there from another side: every load combination in which one of them is loaded
        if len(outs_a) >= 2:
            (c1, d1), (c2, d2) = outs_a[0], outs_a[1]
            for la, lb, rq in (("L", "L", "ab"), ("L", "L", "b"), ("L", "L", "a"), ("L", "U", "a"), ("U", "L", "b"), ("U", "L", "")):
                sa = sid_next() if la == "L" else 0
                sb = sid_next(avoid=[sa]) if lb == "L" else 0
                delivers = lb == "L" and "b" in rq
                P.append(_Proto("goal_moves", f"g{ka}_arrives_as_other_leaves_{la}{lb}_{rq or 'none'}_shelves_{sa}_{sb}",
                                "arrives_as_other_leaves" + (f"+delivery_by_arrival_g{ka}" if delivers else ""),
                                [_Actor(ga, d1, [FORWARD], sa), _Actor(c2, OPP[d2], [FORWARD], sb)],
                                requested=[x for x, r in ((sa, "a"), (sb, "b")) if x and r in rq], unrequested=[x for x, r in ((sa, "a"), (sb, "b")) if x and r not in rq]))
        # the refused swap on the two goal cells
        for la, lb in (("L", "L"), ("L", "U"), ("U", "U")):
            sa = sid_next() if la == "L" else 0
            sb = sid_next(avoid=[sa]) if lb == "L" else 0
            place, extra = {}, ""
            if lb == "U":       # a requested shelf stands under the unloaded one
                sb2 = sid_next(avoid=[sa])
                place, extra = {sb2: gb}, "+delivery_standing_under_unloaded_agent"
            claim = "swap_on_goals" + ("+delivery_in_place" if la == "L" else "") + extra
            P.append(_Proto("goal_moves", f"swap_g{ka}_g{kb}_{la}{lb}_shelves_{sa}_{sb}", claim,
                            [_Actor(ga, d_ab, [FORWARD, FORWARD], sa), _Actor(gb, OPP[d_ab], [FORWARD, NOOP], sb)], place,
                            requested=[x for x in (sa, sb) if x] + list(place)))
        # A follows B across the goals: ga -> gb as B leaves gb
        if outs_b:
            c, d = outs_b[0]
            for la, lb, rq in (("L", "L", "ab"), ("L", "L", "a"), ("L", "U", "a"), ("U", "L", "b"), ("L", "L", "b")):
                sa = sid_next() if la == "L" else 0
                sb = sid_next(avoid=[sa]) if lb == "L" else 0
                delivers = la == "L" and "a" in rq
                P.append(_Proto("goal_moves", f"follow_g{ka}_g{kb}_{la}{lb}_{rq}_shelves_{sa}_{sb}",
                                "follow_across_goals+arrives_as_other_leaves" + (f"+delivery_by_arrival_g{kb}" if delivers else ""),
                                [_Actor(ga, d_ab, [FORWARD], sa), _Actor(gb, d, [FORWARD], sb)],
                                requested=[x for x, r in ((sa, "a"), (sb, "b")) if x and r in rq], unrequested=[x for x, r in ((sa, "a"), (sb, "b")) if x and r not in rq]))

    # ---- 6. a loaded mover faces a cell whose occupant picks up, or unloads, in the same step: the cancel rule reads the occupant's
    #         load at the START of the step (:829-844).  In the toggling step itself the two readings of that rule cannot be told apart
    #         on the reference: the occupant stays on its cell, so the mover stays put whether its move is cancelled (a self-loop of its
    #         own) or refused (an edge into the occupant's self-loop), and ref_step_events counts a failed move either way.  What the
    #         variants below pin is what a kernel can still get wrong there — the mover entering, or a toggle lost, when both happen in
    #         one step — and, `_then_leaves`, that the load the toggle LEFT feeds the rule of the next step: after a pick-up the occupant
    #         walks off loaded and the mover follows into the cell (a rule that still saw a standing shelf under an unloaded occupant
    #         would cancel it); after an unload it walks off unloaded and the mover stays out of the vacated cell for good (a rule that
    #         still saw a loaded occupant would let it follow).  tests/test_shelf_handling.py checks those two outcomes on the recording.
    if N >= 2:
        by_cell = {}
        for c, m, d in g.mover_spots():
            by_cell.setdefault(c, []).append((m, d))
        corner = next(((c, ms) for c, ms in sorted(by_cell.items(), key=lambda kv: (kv[0][1], kv[0][0])) if len(ms) >= 2), None)
        if corner:      # a shelf cell with two highway sides: the mover waits on one, the occupant leaves by the other
            c, ((m, d), (m2, d2)) = corner[0], corner[1][:2]
            s = g.home_at[c]
            sm = sid_next(avoid=[s])
            for flag in (0, 1):
                P.append(_Proto("toggle_vs_mover", f"occupant_picks_then_leaves_{c[0]}_{c[1]}_mover_{sm}_flag{flag}", "pick",
                                [_Actor(m, d, [FORWARD, FORWARD, FORWARD, FORWARD], sm, flag), _Actor(c, OPP[d2], [TOGGLE, FORWARD], 0, flag)], unrequested=[s, sm]))
                P.append(_Proto("toggle_vs_mover", f"occupant_unloads_then_leaves_{c[0]}_{c[1]}_mover_{sm}_flag{flag}", "drop" + (f"+{paid}" if flag else ""),
                                [_Actor(m, d, [FORWARD, FORWARD, FORWARD, FORWARD], sm, 1 - flag), _Actor(c, OPP[d2], [TOGGLE, FORWARD], s, flag)], unrequested=[s, sm]))
        spots = g.mover_spots()
        spots = [spots[i] for i in sorted({0, len(spots) // 2, len(spots) - 1})] if spots else []
        for n, (c, m, d) in enumerate(spots):
            s, sm = g.home_at[c], 0
            sm = sid_next(avoid=[s])
            for flag in (0, 1):
                P.append(_Proto("toggle_vs_mover", f"occupant_picks_{c[0]}_{c[1]}_mover_{sm}_flag{flag}", f"pick+drop@1+pick_nothing|pick@2" + (f"+{paid}@1" if flag else ""),
                                [_Actor(m, d, [FORWARD, FORWARD, FORWARD, FORWARD], sm, flag), _Actor(c, d, [TOGGLE, TOGGLE, TOGGLE], 0, flag)], unrequested=[s, sm]))
                P.append(_Proto("toggle_vs_mover", f"occupant_unloads_{c[0]}_{c[1]}_mover_{sm}_flag{flag}", "drop+pick@1" + (f"+{paid}" if flag else ""),
                                [_Actor(m, d, [FORWARD, FORWARD, FORWARD, FORWARD], sm, 1 - flag), _Actor(c, OPP[d], [TOGGLE, TOGGLE, NOOP], s, flag)], unrequested=[s, sm]))

    # ---- 7. both payments in one reward slot: the last agent unloads with the flag set while a goal nobody stands on pays rewards[-1]
    for k in some_goals:
        for n in range(2):
            s = sid_next()
            s2 = sid_next(avoid=[s])
            extra = [_Actor(quiet[2 % len(quiet)], UP, [TOGGLE], 0, 1)] if n and N >= 2 else []
            P.append(_Proto("payments", f"goal{k}_shelf_{s}_last_unloads_{s2}" + ("_other_toggles" if extra else ""), "both_payments_one_slot+drop+delivery_nobody_on_goal",
                            [_Actor(g.home[s2], UP, [TOGGLE, TOGGLE, TOGGLE], s2, 1)] + extra, {s: g.goals[k]}, requested=[s], unrequested=[s2], pin_last=0))

    # ---- 8. the limits: counters injected next to LIMITS (and near 2^30 for the configuration without limits), with no delivery, a
    #         delivery at step 0 (nobody on the goal: no register of any lane knows of it) and one at step 1 (by arrival)
    MS, MI = LIMITS["max_steps"], LIMITS["max_inactivity_steps"]
    big = "U:max_steps_none_counter_near_2_30+U:max_inactivity_steps_none_counter_near_2_30"
    counters = [("steps_due", MS - 1, 0, "L:max_steps_due_{how}"), ("steps_one_before", MS - 2, 0, "L:max_steps_one_before+L:max_steps_due_{how1}@1"),
                ("inactivity_due", 0, MI - 1, "L:max_inactivity_steps_due_{how}"),
                ("inactivity_one_before", 0, MI - 2, "L:max_inactivity_steps_one_before|max_inactivity_steps_due_with_delivery@{t1}"),
                ("both_due", MS - 1, MI - 1, "L:both_limits_due+L:max_steps_due_{how}+L:max_inactivity_steps_due_{how}"),
                ("both_one_before", MS - 2, MI - 2, "L:max_steps_one_before"), ("steps_past", MS + 3, 1, "L:max_steps_due_{how}"),
                ("inactivity_past", 2, MI + 2, "L:max_inactivity_steps_due_{how}"),
                ("near_2_30", (1 << 30) - 3, (1 << 30) - 2, big), ("near_2_30_steps_only", (1 << 30) - 1, 0, "U:max_steps_none_counter_near_2_30")]
    for n, (name, st, ina, claim) in enumerate(counters):
        for when in ("none", "step0", "step1"):
            k = (n + len(when)) % len(g.goals)
            s = sid_next()
            if when == "none":
                actors, place, req = [], {}, []
            elif when == "step0":
                actors, place, req = [], {s: g.goals[k]}, [s]
            else:
                ap = g.approaches(g.goals[k])
                if not ap:
                    continue
                actors, place, req = [_Actor(ap[0][0], ap[0][1], [NOOP, FORWARD], s)], {}, [s]
            cl = claim.format(how="with_delivery" if when == "step0" else "without_delivery", how1="with_delivery" if when == "step1" else "without_delivery",
                              t1=0 if when == "none" else 1)
            if name == "inactivity_one_before" and when == "step0":
                cl = "delivery_nobody_on_goal"
            P.append(_Proto("limits", f"{name}_delivery_{when}", cl + ("+delivery_nobody_on_goal" if when == "step0" else ""), actors, place, requested=req,
                            steps=st, inactive=ina))

    # ---- 9. the whole story where a shelf cell lies straight behind a goal: deliver, carry off, unload (paid), re-pick, unload (unpaid)
    for k, a, d, h in g.story_spots():
        s = g.home_at[h]
        P.append(_Proto("story", f"g{k}_from_{a[0]}_{a[1]}_shelf_{s}", f"delivery_by_arrival_g{k}+loaded_leaves_goal@1+drop@2+pick@3+drop@4",
                        [_Actor(a, d, [FORWARD, FORWARD, TOGGLE, TOGGLE, TOGGLE], s)], requested=[s]))
    return [p for p in P if len(p.actors) <= N and len(p.requested) <= Q]


def _ids_for(assignment, k, N, pin_last):
    if assignment == "lowest":
        order = list(range(N))
    elif assignment == "highest":
        order = list(range(N - 1, -1, -1))
    else:
        a, b = (int(v) for v in assignment[1:].split("_"))
        if b >= N:
            return None
        order = [v for pair in zip(range(a, -1, -1), range(b, N)) for v in pair]
        order += [v for v in range(N) if v not in order]
    if pin_last is None:
        return order[:k]
    rest = [v for v in order if v != N - 1][:k - 1]
    return rest[:pin_last] + [N - 1] + rest[pin_last:]


def _emit(g, shape, proto, assignment, ids, number):
    N, S, Q = g.N, g.S, g.Q
    ax, ay, ad, ac, af = (np.zeros(N, np.int32) for _ in range(5))
    actions = np.zeros((T_STEPS, N), np.int32)
    pos = dict(g.home)                      # shelf id -> cell
    at = dict(g.home_at)

    def put(s, cell):
        other, old = at.get(cell), pos[s]
        if other == s:
            return
        at.pop(old, None)
        pos[s], at[cell] = cell, s
        if other:
            pos[other], at[old] = old, other

    foot = set(g.goals)
    for gc in g.goals:
        foot.update(g.step(gc, d) for d in DXY)
    for s, cell in proto.place.items():
        put(s, cell)
        foot.add(cell)
    for actor, i in zip(proto.actors, ids):
        ax[i], ay[i], ad[i], ac[i], af[i] = actor.cell[0], actor.cell[1], actor.dir, actor.carry, actor.flag
        actions[:, i] = actor.acts
        if actor.carry:
            put(actor.carry, actor.cell)
        c, d = actor.cell, actor.dir
        foot.add(c)
        for a in actor.acts:
            if a == FORWARD:
                c = (min(max(c[0] + DXY[d][0], 0), g.W - 1), min(max(c[1] + DXY[d][1], 0), g.H - 1))
                foot.add(c)
            d = _TURN_L[d] if a == TURN_LEFT else _TURN_R[d] if a == TURN_RIGHT else d
    touched = set(proto.place) | {a.carry for a in proto.actors if a.carry} | set(proto.requested) | set(proto.unrequested)
    foot.update(g.home[s] for s in touched)
    foot.update(pos[s] for s in touched)
    # everybody else: NOOP on the left wall, then on the right wall, the top row and whatever else is free
    cells = [(0, y) for y in range(g.H)] + [(g.W - 1, y) for y in range(g.H)] + [(x, 0) for x in range(g.W)] + [(x, y) for y in range(g.H) for x in range(g.W)]
    free = [c for c in dict.fromkeys(cells) if c not in foot]
    parked = [i for i in range(N) if i not in ids]
    assert len(free) >= len(parked), (proto.variant, len(free), len(parked))
    for i, c in zip(parked, free):
        ax[i], ay[i], ad[i] = c[0], c[1], UP
    # the queue: the reset's, with what must not be requested taken out and what must be put in (the slot moves with the scenario)
    base = [int(q) for q in shape["queue"]]
    queue = [q if q not in touched else 0 for q in base]
    fill = (s for s in range(1 + number % 7, S + 1) if s not in base and s not in touched)
    queue = [q or next(fill) for q in queue]
    for n, s in enumerate(proto.requested):
        queue[(number + n) % Q] = s
    assert len(set(queue)) == Q and not set(queue) & set(proto.unrequested), (proto.variant, queue)
    # the generator state: the reset's, or one whose next draws return the chosen replacements
    rng = np.array(shape["rng0"], np.uint64)
    if proto.draws:
        inc = (int(rng[2]) << 64) | int(rng[3])
        q, vals = list(queue), []
        for delivered, new in proto.draws:
            cand = [s for s in range(1, S + 1) if s not in q]
            vals.append(rs.accepted_value(S - Q, cand.index(new)))
            q[q.index(delivered)] = new
        rng = rs._state(inc, 0, 0, vals[0], vals[1] if len(vals) > 1 else rs.SAFE)
    shelf_xy = np.array([pos[s] for s in range(1, S + 1)], np.int32)
    assert len({tuple(c) for c in shelf_xy}) == S and len({(int(x), int(y)) for x, y in zip(ax, ay)}) == N, proto.variant
    return dict(family=proto.family, variant=proto.variant, claim=proto.claim, ids=assignment, agent_x=ax, agent_y=ay, agent_dir=ad, agent_carry=ac,
                agent_delivered=af, shelf_xy=shelf_xy, queue=np.array(queue, np.int32), steps=np.int32(proto.steps), inactive=np.int32(proto.inactive),
                rng=rng, actions=actions)


def build_scenarios(shape, seed=0):
    """Scenarios for one task.  Every situation comes with the acting agents on the lowest ids; the other assignments of
    ID_ASSIGNMENTS that N admits go round the situations of each family, every situation taking at least one of them and every family
    seeing all of them (`seed` turns the round).  Situations without an acting agent come once."""
    g = _Geo(shape)
    N = g.N
    protos = _protos(g, shape)
    others = [a for a in ID_ASSIGNMENTS[1:] if N >= 2 and (a == "highest" or int(a[1:].split("_")[1]) < N)]
    out = []
    for fam in FAMILIES:
        ps = [p for p in protos if p.family == fam]
        acting = [p for p in ps if p.actors]
        plan = [(p, "lowest") for p in ps]
        if acting and others:
            plan += [(acting[j % len(acting)], others[(j + seed) % len(others)]) for j in range(max(len(acting), len(others)))]
        for p, a in plan:
            ids = _ids_for(a, len(p.actors), N, p.pin_last)
            out.append(_emit(g, shape, p, a, ids, len(out)))
    return out
