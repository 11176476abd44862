"""Constructed collision structures for the step kernels, and a census that names what a move graph holds.

The reference resolves one step's moves with a networkx graph (rware/warehouse.py:821-876): cell -> requested cell per agent,
`find_cycle` per weakly connected component, else `dag_longest_path`.  The kernels run a closed form of that rule in three texts
(register exchange, per-cell LDS exchange, generic kernel).  Random play hardly ever builds the rare structures, so this module
BUILDS them — chains of every length, blocked heads, cycles with and without tails, refused 2-swaps, junctions of every depth
combination, nested junctions, the loaded-agent rules at the target cell — under several agent-id assignments, so that every bit
field of the kernels' link / priority words sees a chain member.

Plain numpy and dicts; no networkx.  Two entry points:

  build_scenarios(base, seed)   -> list of scenario dicts (full injected state of ONE env + 4 steps of actions)
  census(state, actions, H, W, shelf_layer) -> Counter of structure classes of one env's move graph, after the shelf-block cancel

`analyse` (what `census` wraps) also predicts WHO moves under the pinned tie rule (lowest agent id among equal-depth predecessors):
tests compare that prediction with the live reference, so the classifier is itself a checked thing.
"""
from collections import Counter

import numpy as np

UP, DOWN, LEFT, RIGHT = 0, 1, 2, 3
NOOP, FORWARD, TURN_LEFT, TURN_RIGHT, TOGGLE = 0, 1, 2, 3, 4
DXY = {UP: (0, -1), DOWN: (0, 1), LEFT: (-1, 0), RIGHT: (1, 0)}
OPP = {UP: DOWN, DOWN: UP, LEFT: RIGHT, RIGHT: LEFT}
_TURN_L = {UP: LEFT, LEFT: DOWN, DOWN: RIGHT, RIGHT: UP}
_TURN_R = {v: k for k, v in _TURN_L.items()}
T_STEPS = 4

FAMILIES = ("chain", "blocked_head", "cycle", "swap", "junction", "head_loses", "loaded")
ID_ASSIGNMENTS = ("ascending", "descending", "random", "boundary")


def name_of(task, z, k, t):
    """Scenario k of a recorded fixture of these scenarios (tests/golden/collisions, tests/golden/wide/collisions-straddle) at step t."""
    return (f"{task}, scenario {k} ({FAMILIES[z['family'][k]]} / {z['variant'][k]}, claims {z['claim'][k]}), "
            f"ids {ID_ASSIGNMENTS[z['ids'][k]]}, step {t}")


# ------------------------------------------------------------------------------------------------------------------ census
def analyse(ax, ay, ad, ac, actions, H, W, shelf_layer):
    """(Counter of classes, set of agents that change cell this step) for one env.  `shelf_layer`: (H, W) shelf ids at the START
    of the step (carried shelves included, as `_recalc_grid` leaves them).  Classes, one count per weakly connected component
    unless said otherwise:
      cycle_k / cycle_k_tail        k >= 3 agents rotate; _tail: more agents feed the cycle (they fail)
      swap / swap_tail              a 2-cycle: refused, nobody moves
      chain_d                       a component draining into an empty cell: d followers move behind the head (d = 0: a lone mover)
      chain_blocked_stationary      >= 1 follower behind an agent that stays (NOOP, turn, TOGGLE_LOAD, wall clamp)
      chain_blocked_shelf           ... behind a loaded agent whose FORWARD was cancelled by a standing shelf
      junction_unequal / junction_tie   per cell of a draining component with >= 2 entrants: deepest entrant unique / not
      junction_nested               a draining component with >= 2 such cells
      head_loses                    per losing entrant of a junction that has followers of its own (they all fail)
      loaded_follows_loaded         per loaded agent that enters a shelf-holding cell because its occupant is loaded (:833-838)
    """
    N = len(ax)
    pos = [(int(ax[i]), int(ay[i])) for i in range(N)]
    at = {p: i for i, p in enumerate(pos)}
    assert len(at) == N, "two agents on one cell"
    tgt, cancelled = [], [False] * N
    out = Counter()
    for i in range(N):
        t = pos[i]
        if int(actions[i]) == FORWARD:
            dx, dy = DXY[int(ad[i])]
            t = (min(max(pos[i][0] + dx, 0), W - 1), min(max(pos[i][1] + dy, 0), H - 1))
        if ac[i] and t != pos[i] and shelf_layer[t[1], t[0]]:
            j = at.get(t)
            if j is not None and ac[j]:
                out["loaded_follows_loaded"] += 1
            else:
                cancelled[i], t = True, pos[i]
        tgt.append(t)
    preds = {}
    for i in range(N):
        if tgt[i] != pos[i]:
            preds.setdefault(tgt[i], []).append(i)

    def terminal(i):
        seen, cur = [], i
        while True:
            if cur in seen:
                return ("cycle", tuple(sorted(seen[seen.index(cur):])))
            seen.append(cur)
            if tgt[cur] == pos[cur]:
                return ("stay", cur)
            nxt = at.get(tgt[cur])
            if nxt is None:
                return ("sink", tgt[cur])
            cur = nxt

    groups = {}
    for i in range(N):
        groups.setdefault(terminal(i), []).append(i)
    depth_memo = {}

    def depth(i):
        if i not in depth_memo:
            depth_memo[i] = 1 + max((depth(p) for p in preds.get(pos[i], ())), default=-1)
        return depth_memo[i]

    movers = set()
    for (kind, key), members in groups.items():
        if kind == "stay":
            if len(members) > 1:
                out["chain_blocked_shelf" if cancelled[key] else "chain_blocked_stationary"] += 1
        elif kind == "cycle":
            k, tail = len(key), "_tail" if len(members) > len(key) else ""
            if k == 2:
                out["swap" + tail] += 1
            else:
                out[f"cycle_{k}{tail}"] += 1
                movers.update(key)
        else:
            cell, path = key, []
            while preds.get(cell):
                w = min(preds[cell], key=lambda p: (-depth(p), p))
                path.append(w)
                cell = pos[w]
            movers.update(path)
            out[f"chain_{len(path) - 1}"] += 1
            n_junctions = 0
            for c in [key] + [pos[m] for m in members]:
                ps = preds.get(c, ())
                if len(ps) < 2:
                    continue
                n_junctions += 1
                ds = sorted((depth(p) for p in ps), reverse=True)
                out["junction_unequal" if ds[0] > ds[1] else "junction_tie"] += 1
                w = min(ps, key=lambda p: (-depth(p), p))
                out["head_loses"] += sum(1 for p in ps if p != w and depth(p) >= 1)
            if n_junctions >= 2:
                out["junction_nested"] += 1
    return +out, movers


def census(state, actions, H, W, shelf_layer):
    """Counter of structure classes of ONE env: `state` holds agent_x / agent_y / agent_dir / agent_carry (N,) at the start of
    the step, `shelf_layer` the (H, W) shelf ids then."""
    return analyse(state["agent_x"], state["agent_y"], state["agent_dir"], state["agent_carry"], actions, H, W, shelf_layer)[0]


def shelf_layer_from_xy(shelf_xy, H, W):
    layer = np.zeros((H, W), np.int32)
    sx = np.asarray(shelf_xy)
    layer[sx[:, 1], sx[:, 0]] = np.arange(1, len(sx) + 1)
    return layer


def class_matches(counter, claim):
    """`claim`: class names joined by '+'; a trailing '*' matches any suffix (`cycle_*` ...)."""
    for c in claim.split("+"):
        if c == "nothing":
            if counter:
                return False
        elif c.endswith("*"):
            if not any(k.startswith(c[:-1]) and not k[len(c) - 1:].endswith("_tail") for k in counter):
                return False
        elif counter.get(c, 0) < 1:
            return False
    return True


# --------------------------------------------------------------------------------------------------------------- generator
def _step(c, d, k=1):
    return (c[0] + DXY[d][0] * k, c[1] + DXY[d][1] * k)


def _dir_to(a, b):
    for d, (dx, dy) in DXY.items():
        if (a[0] + dx, a[1] + dy) == b:
            return d
    raise AssertionError((a, b))


def _grow(start, d, n, used, H, W, bend=0):
    """n cells from `start` (excluded) in direction d, straight while it can — or, `bend` > 0, turning every `bend` cells,
    left and right in turn — a simple path that stays on the grid and off `used`; None if there is none."""
    out, taken = [], set(used)
    taken.add(start)

    def rec(c, d, run, flip):
        if len(out) == n:
            return True
        first, second = (_TURN_L[d], _TURN_R[d]) if flip else (_TURN_R[d], _TURN_L[d])
        order = [first, second, d] if bend and run >= bend else [d, first, second]
        for nd in order:
            nc = _step(c, nd)
            if 0 <= nc[0] < W and 0 <= nc[1] < H and nc not in taken:
                out.append(nc)
                taken.add(nc)
                if rec(nc, nd, run + 1 if nd == d else 1, (not flip) if nd != d else flip):
                    return True
                taken.discard(out.pop())
        return False

    return out if rec(start, d, 0, False) else None


class _Proto:
    """One structure before ids are assigned: slots in structure order (cell, dir, action, loaded)."""

    def __init__(self, family, variant, claim):
        self.family, self.variant, self.claim = family, variant, claim
        self.slots = []

    def add(self, cell, d, act=FORWARD, loaded=False):
        assert all(s[0] != cell for s in self.slots), (self.variant, cell)
        self.slots.append((cell, d, act, loaded))
        return self

    def chain(self, toward, cells, loaded=False):
        """Agents on `cells`, each facing the one before it; the first faces `toward`."""
        prev = toward
        for c in cells:
            self.add(c, _dir_to(c, prev), FORWARD, loaded)
            prev = c
        return self


def _protos(H, W, N):
    P = []

    def inb(c):
        return 0 <= c[0] < W and 0 <= c[1] < H

    # ---- 1. chains draining into an empty cell: k agents (k - 1 followers), straight (bending where the grid ends) and bent
    starts = [((3, 0), DOWN), ((W - 1, 3), LEFT), ((6, H - 1), UP), ((0, 6), RIGHT)]
    for k in range(1, N + 1):
        c0, d = starts[k % 4]
        cells = _grow(c0, d, k, (), H, W)
        P.append(_Proto("chain", f"straight_{k}", f"chain_{k - 1}").chain(c0, cells))
        if k >= 3:
            cells = _grow((4, 5), (UP, RIGHT, DOWN, LEFT)[k % 4], k, (), H, W, bend=1 + k % 2)
            P.append(_Proto("chain", f"bent_{k}", f"chain_{k - 1}").chain((4, 5), cells))

    # ---- 2. the same chains behind a head that does not move
    heads = [("noop", (3, 4), UP, NOOP, DOWN), ("turn_left", (3, 4), LEFT, TURN_LEFT, RIGHT), ("turn_right", (6, 4), UP, TURN_RIGHT, LEFT),
             ("toggle", (3, 5), DOWN, TOGGLE, UP), ("toggle_on_shelf", (2, 4), LEFT, TOGGLE, RIGHT),
             ("wall_up", (3, 0), UP, FORWARD, DOWN), ("wall_down", (6, H - 1), DOWN, FORWARD, UP),
             ("wall_left", (0, 4), LEFT, FORWARD, RIGHT), ("wall_right", (W - 1, 4), RIGHT, FORWARD, LEFT),
             ("shelf", (3, 4), LEFT, FORWARD, RIGHT)]
    for name, hc, hd, act, grow_d in heads:
        for k in range(2, N + 1):
            cells = _grow(hc, grow_d, k - 1, (), H, W, bend=0 if k % 3 else 2)
            p = _Proto("blocked_head", f"{name}_{k}", "chain_blocked_shelf" if name == "shelf" else "chain_blocked_stationary")
            p.add(hc, hd, act, loaded=(name == "shelf")).chain(hc, cells)
            P.append(p)

    # ---- 3. cycles: rectangle rings of 4, 6, 8, ... agents, both senses; bare, loaded, with one and two tails
    def ring(ox, oy, w, h):
        top = [(ox + i, oy) for i in range(w)]
        right = [(ox + w - 1, oy + j) for j in range(1, h)]
        bottom = [(ox + i, oy + h - 1) for i in range(w - 2, -1, -1)]
        left = [(ox, oy + j) for j in range(h - 2, 0, -1)]
        return top + right + bottom + left   # clockwise on the screen (y grows downwards)

    def tails_for(cells, lengths):
        """One straight tail per requested length, each into a different ring cell, from outside; None if they do not fit."""
        used, out = set(cells), []
        order = list(range(len(cells)))
        for n_t, L in enumerate(lengths):
            found = None
            for idx in (order if n_t == 0 else order[len(order) // 2:] + order[:len(order) // 2]):
                if any(idx == o[0] for o in out):
                    continue
                for d in (LEFT, UP, RIGHT, DOWN):
                    t = [_step(cells[idx], d, j) for j in range(1, L + 1)]
                    if all(inb(c) and c not in used for c in t):
                        found = (idx, t)
                        break
                if found:
                    break
            if not found:
                return None
            used.update(found[1])
            out.append(found)
        return out

    shapes = {}
    for k in range(4, N + 1, 2):
        cand = [(2, k // 2)] + [(w, k // 2 + 2 - w) for w in (3, 4) if k // 2 + 2 - w >= w]
        shapes[k] = [(w, h) for w, h in cand if h <= H - 2 and w <= W - 4][:2]
    for k, whs in shapes.items():
        for (w, h) in whs:
            base_cells = ring(3, 1, w, h)
            for sense in ("cw", "ccw"):
                cells = base_cells if sense == "cw" else base_cells[::-1]

                def cyc(variant, claim, loaded=False, tails=()):
                    p = _Proto("cycle", f"{w}x{h}_{sense}_{variant}", claim)
                    for i, c in enumerate(cells):
                        p.add(c, _dir_to(c, cells[(i + 1) % k]), FORWARD, loaded)
                    for idx, t in tails:
                        p.chain(cells[idx], t)
                    return p

                P.append(cyc("bare", f"cycle_{k}"))
                P.append(cyc("loaded", f"cycle_{k}+loaded_follows_loaded", loaded=True))
                for lengths in [(1,), (2,), (3,), (1, 1), (2, 2), (3, 3), (1, 3)]:
                    if k + sum(lengths) > N:
                        continue
                    ts = tails_for(cells, lengths)
                    if ts:
                        P.append(cyc("tail" + "_".join(map(str, lengths)), f"cycle_{k}_tail", tails=ts))

    # ---- 4. 2-swaps (refused), bare and with tails on one and on both sides, loaded and not
    for n_o, (a, da) in enumerate([((4, 0), RIGHT), ((3, 5), DOWN)]):
        b = _step(a, da)
        for ta, tb in [(0, 0), (1, 0), (2, 0), (3, 0), (0, 2), (1, 1), (2, 2), (3, 3), (1, 3)]:
            if 2 + ta + tb > N:
                continue
            for load in ("none", "one", "both", "all"):
                if n_o == 1 and load in ("both", "all"):
                    continue   # (the vertical one crosses shelf rows: a loaded tail there is the shelf-block case of family 7)
                p = _Proto("swap", f"{'hv'[n_o]}_{ta}_{tb}_{load}", "swap_tail" if ta + tb else "swap")
                p.add(a, da, FORWARD, load != "none").add(b, OPP[da], FORWARD, load in ("both", "all"))
                p.chain(a, [_step(a, OPP[da], j) for j in range(1, ta + 1)], loaded=(load == "all"))
                p.chain(b, [_step(b, da, j) for j in range(1, tb + 1)], loaded=(load == "all"))
                P.append(p)

    # ---- 5. junctions: branches of given depths into one empty cell; branch order = id order of the heads
    def junction(J, dirs, depths, order, variant, claim=None, family="junction", extra=None):
        used, branches = {J}, []
        for d, dep in zip(dirs, depths):
            cells = _grow(J, d, dep + 1, used, H, W)
            if cells is None or cells[0] != _step(J, d):
                return None
            used.update(cells)
            branches.append(cells)
        if sum(len(b) for b in branches) + (len(extra[1]) if extra else 0) > N:
            return None
        if claim is None:
            ds = sorted(depths, reverse=True)
            claim = "junction_unequal" if ds[0] > ds[1] else "junction_tie"
            if any(dep >= 1 for dep in ds[1:]) and ds[0] > ds[1]:
                claim += "+head_loses"
        p = _Proto(family, variant, claim)
        for b in order:
            p.chain(J, branches[b])
        if extra:   # a side chain into the cell of member `extra[0]` = (branch, index)
            (b, i), cells = extra
            if any(c in used or not inb(c) for c in cells):
                return None
            p.chain(branches[b][i], cells)
        return p

    def perms(n):
        return [(0, 1), (1, 0)] if n == 2 else [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]

    J0 = (4, 5)
    for n_pair, dirs in enumerate([(LEFT, UP), (LEFT, RIGHT)]):
        for d1 in range(4):
            for d2 in range(4):
                if (d1 + d2) % 2 != n_pair and (d1, d2) not in ((1, 1), (2, 3)):
                    continue   # (perpendicular and opposite branches share the 16 combinations; two of them run on both)
                for o in perms(2):
                    P.append(junction(J0, dirs, (d1, d2), o, f"2b_{'LU' if n_pair == 0 else 'LR'}_{d1}{d2}_o{o[0]}{o[1]}"))
    for d1 in range(4):
        for d2 in range(4):
            for d3 in range(4):
                for o in perms(3):
                    P.append(junction(J0, (LEFT, UP, RIGHT), (d1, d2, d3), o, f"3b_{d1}{d2}{d3}_o{''.join(map(str, o))}"))
    for o in perms(2):   # the deep case: N - 2 followers against none
        P.append(junction(J0, (LEFT, UP), (N - 2, 0), o, f"deep_{N - 2}_0_o{o[0]}{o[1]}"))
        P.append(junction(J0, (UP, LEFT), (N - 2, 0), o, f"deep_up_{N - 2}_0_o{o[0]}{o[1]}"))
    borders = [("corner_tl", (0, 0), (RIGHT, DOWN)), ("corner_tr", (W - 1, 0), (LEFT, DOWN)), ("corner_bl", (0, H - 1), (RIGHT, UP)),
               ("corner_br", (W - 1, H - 1), (LEFT, UP)), ("border_t", (4, 0), (LEFT, RIGHT, DOWN)), ("border_b", (3, H - 1), (LEFT, RIGHT, UP)),
               ("border_l", (0, 5), (UP, DOWN, RIGHT)), ("border_r", (W - 1, 5), (UP, DOWN, LEFT))]
    for name, J, dirs in borders:
        combos = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 1), (1, 2), (3, 3), (0, 3)] if len(dirs) == 2 else \
                 [(0, 0, 0), (1, 0, 2), (2, 1, 0), (1, 1, 1), (0, 2, 2), (3, 1, 3)]
        for depths in combos:
            for o in perms(len(dirs)):
                P.append(junction(J, dirs, depths, o, f"{name}_{''.join(map(str, depths))}_o{''.join(map(str, o))}"))
    # nested: a side chain of depth s enters the cell of member 1 of a branch of `main` + 1 agents (main - 2 followers' depth behind
    # that cell), in the branch that wins the outer junction (other branch shallower) and in the one that loses it (other deeper)
    for main in (3, 2):
        for where, other_depth in (("winner", main - 2), ("loser", main + 1)):
            for s in range(3):
                for side in (UP, DOWN):
                    for o in perms(2):
                        m1 = _step(J0, LEFT, 2)
                        cells = [_step(m1, side, j) for j in range(1, s + 2)]
                        claim = "junction_nested+" + ("junction_tie" if s == main - 2 else "junction_unequal")
                        P.append(junction(J0, (LEFT, RIGHT), (main, other_depth), o, f"nested_{where}_m{main}_s{s}_{'ud'[side]}_o{o[0]}{o[1]}",
                                          claim=claim, extra=((0, 1), cells)))

    # ---- 6. head loses, chain fails: k agents against k + 1 into one cell
    for k in range(1, (N - 1) // 2 + 1):
        for o in perms(2):
            P.append(junction(J0, (LEFT, UP) if k % 2 else (DOWN, RIGHT), (k - 1, k), o, f"k{k}_o{o[0]}{o[1]}",
                              claim="junction_unequal" + ("+head_loses" if k >= 2 else ""), family="head_loses"))

    # ---- 7. loaded-agent rules at the target cell (cells (1, y), (2, y), y in 1..8: shelf columns of every registered size)
    if N >= 2:
        for occ_act, name in ((FORWARD, "leader_moves"), (NOOP, "leader_stays"), (TOGGLE, "leader_unloads")):
            # loaded follower into a shelf-column cell whose shelf its loaded occupant carries: the edge stays (:833-838)
            p = _Proto("loaded", f"follows_loaded_{name}", "loaded_follows_loaded" + ((f"+chain_{min(N, 3) - 1}") if occ_act == FORWARD else "+chain_blocked_stationary"))
            p.add((1, 3), LEFT, occ_act, True).add((2, 3), LEFT, FORWARD, True)
            if N >= 3:
                p.add((3, 3), LEFT, FORWARD, False)
            P.append(p)
        for occ_act, name in ((FORWARD, "occupant_leaves"), (NOOP, "occupant_stays"), (TOGGLE, "occupant_loads")):
            # loaded into a cell with a standing shelf and an unloaded agent: cancelled, whatever the occupant does (start-of-step values)
            p = _Proto("loaded", f"standing_shelf_{name}", "chain_blocked_shelf" if N >= 3 else "chain_0" if occ_act == FORWARD else "nothing")
            p.add((1, 5), LEFT, occ_act, False).add((2, 5), LEFT, FORWARD, True)
            if N >= 3:
                p.add((3, 5), LEFT, FORWARD, False)
            P.append(p)
        for k in range(2, min(N, 8) + 1):   # a loaded chain up a shelf column and out onto the highway row
            p = _Proto("loaded", f"column_chain_{k}", f"chain_{k - 1}+loaded_follows_loaded")
            p.chain((1, 0), [(1, y) for y in range(1, k + 1)], loaded=True)
            P.append(p)
        for k in range(2, min(N, 4) + 1):   # ... and along a shelf row out to the highway column: (1, 7) .. (k, 7) -> (0, 7)
            p = _Proto("loaded", f"row_chain_{k}", f"chain_{k - 1}+loaded_follows_loaded")
            p.chain((0, 7), [(x, 7) for x in range(1, k + 1)], loaded=True)
            P.append(p)
    return [p for p in P if p is not None and len(p.slots) <= N]


def _boundary_order(N, rot):
    """Agent ids with consecutive structure slots on both sides of every encoding boundary that exists for N: 5|6 (32- / 64-bit
    links from 7 agents), 11|12, 12|13 (64 / 128 bits), 15|16 (4- / 5-bit priority fields), and the last index."""
    groups = [g for g in ([i for i in g if i < N] for g in ([5, 6], [11, 12, 13], [15, 16], [N - 1, 0])) if len(g) >= 2]
    groups = groups[rot % len(groups):] + groups[:rot % len(groups)]
    out = []
    for g in groups:
        out += [i for i in g if i not in out]
    return out + [i for i in range(N) if i not in out]


def _emit(proto, ids, assignment, base, H, W, N):
    n = len(proto.slots)
    cells = [s[0] for s in proto.slots]
    foot = set(cells)
    for c, d, act, _ in proto.slots:
        foot.add((min(max(c[0] + DXY[d][0], 0), W - 1), min(max(c[1] + DXY[d][1], 0), H - 1)))
    free = [(x, y) for y in range(H) for x in range(W) if (x, y) not in foot]
    free.sort(key=lambda c: (-min(abs(c[0] - f[0]) + abs(c[1] - f[1]) for f in foot), c[1], c[0]))
    parked = [i for i in range(N) if i not in ids]
    ax, ay, ad, ac = (np.zeros(N, np.int32) for _ in range(4))
    act0 = np.zeros(N, np.int32)
    shelf_xy = np.array(base["shelf_xy"], np.int32).copy()
    shelf_at = {(int(x), int(y)): s for s, (x, y) in enumerate(shelf_xy)}
    queue = set(int(q) for q in base["queue"])
    # shelves a loaded agent on a shelf-less cell takes along: unrequested ones first (a requested one may be delivered on the way)
    spare = [s for s in range(len(shelf_xy) - 1, -1, -1) if tuple(shelf_xy[s]) not in foot]
    spare.sort(key=lambda s: (s + 1) in queue)
    for (c, d, act, loaded), i in zip(proto.slots, ids):
        ax[i], ay[i], ad[i], act0[i] = c[0], c[1], d, act
        if loaded:
            s = shelf_at.get(c)
            if s is None:
                s = spare.pop(0)
                del shelf_at[tuple(shelf_xy[s])]
                shelf_xy[s] = c
                shelf_at[c] = s
            ac[i] = s + 1
    for i, c in zip(parked, free):
        ax[i], ay[i], ad[i] = c[0], c[1], UP
    actions = np.full((T_STEPS, N), FORWARD, np.int32)
    actions[0] = act0
    return dict(family=proto.family, variant=proto.variant, claim=proto.claim, ids=assignment, agent_x=ax, agent_y=ay, agent_dir=ad,
                agent_carry=ac, agent_delivered=np.zeros(N, np.int32), shelf_xy=shelf_xy, queue=np.array(base["queue"], np.int32),
                actions=actions)


def build_scenarios(base, seed=0, cap=None):
    """Scenarios for one task.  `base`: dict(H, W, N, shelf_xy (S, 2) per shelf id, queue (Q,)) — the state a
    seeded reset() gave.  Every structure comes under the ascending id assignment; the descending, seeded-random and boundary
    assignments of families 1-6 and the junction family are thinned by a seeded sample down to `cap` scenarios in all (never to
    zero per family and assignment)."""
    H, W, N = int(base["H"]), int(base["W"]), int(base["N"])
    protos = _protos(H, W, N)
    rng = np.random.default_rng(seed)
    core, pool = [], []
    for k, p in enumerate(protos):
        n = len(p.slots)
        assigns = [("ascending", list(range(n)))]
        if p.family != "loaded":
            assigns += [("descending", list(range(N - 1, N - 1 - n, -1))), ("random", [int(v) for v in rng.permutation(N)[:n]]),
                        ("boundary", _boundary_order(N, k)[:n])]
        for name, ids in assigns:
            keep = name == "ascending" and p.family != "junction"
            (core if keep else pool).append((p, name, ids))
    if cap is not None and len(core) + len(pool) > cap:
        # one of every (family, assignment) first, then a seeded sample of the rest
        first, seen = [], set()
        for item in pool:
            key = (item[0].family, item[1], item[0].claim)
            if key not in seen:
                seen.add(key)
                first.append(item)
        rest = [it for it in pool if not any(it is f for f in first)]
        n_more = max(0, cap - len(core) - len(first))
        pick = sorted(rng.choice(len(rest), size=min(n_more, len(rest)), replace=False).tolist()) if n_more else []
        pool = first + [rest[i] for i in pick]
    return [_emit(p, ids, name, base, H, W, N) for p, name, ids in core + pool]


# ------------------------------------------------------------------------------------------------- dense re-packing (floor test)
def pack_dense(rng, ax, ay, ad, ac, shelf_layer, H, W):
    """New (x, y, dir) for the N agents of one env inside a random 4x5 .. 5x6 block.  Uniformly random directions alone cannot
    reach a chain of N / 2 followers (each link is right with probability 1 / 4: 4^-9 for ten agents), so two packs in three
    lay the agents along a structure and leave only a few directions to chance: a random walk through the block (long chains,
    junctions where the strays point into it), or a rectangle ring with the others feeding it (cycles with tails).  Loaded
    agents keep their shelves and only go to cells without a standing shelf."""
    N = len(ax)
    carried = set(int(c) for c in ac if c)
    for _ in range(200):
        bh, bw = (int(rng.integers(4, 6)), int(rng.integers(5, 7)))
        if rng.random() < 0.5:
            bh, bw = bw, bh
        if bh > H or bw > W or bh * bw < N + 1:
            continue
        oy, ox = int(rng.integers(0, H - bh + 1)), int(rng.integers(0, W - bw + 1))
        block = [(x, y) for y in range(oy, oy + bh) for x in range(ox, ox + bw)]
        ok_loaded = {c for c in block if shelf_layer[c[1], c[0]] == 0 or int(shelf_layer[c[1], c[0]]) in carried}
        mode = int(rng.integers(0, 3))
        cells, dirs = None, None
        if mode == 1:
            start = block[int(rng.integers(len(block)))]
            walk = _grow(start, int(rng.integers(0, 4)), N, [c for c in [(x, y) for y in range(-1, H + 1) for x in range(-1, W + 1)]
                                                               if c not in block], H, W, bend=int(rng.integers(0, 4)))
            if walk is None:
                continue
            cells = walk
            dirs = [_dir_to(walk[0], start)] + [_dir_to(walk[i], walk[i - 1]) for i in range(1, N)]
        elif mode == 2:
            w, h = int(rng.integers(2, 4)), int(rng.integers(2, 4))
            k = 2 * (w + h) - 4
            if k > N or w > bw or h > bh:
                continue
            rx, ry = ox + int(rng.integers(0, bw - w + 1)), oy + int(rng.integers(0, bh - h + 1))
            top = [(rx + i, ry) for i in range(w)]
            ring = top + [(rx + w - 1, ry + j) for j in range(1, h)] + [(rx + i, ry + h - 1) for i in range(w - 2, -1, -1)] + \
                [(rx, ry + j) for j in range(h - 2, 0, -1)]
            if rng.random() < 0.5:
                ring = ring[::-1]
            cells = list(ring)
            dirs = [_dir_to(c, ring[(i + 1) % k]) for i, c in enumerate(ring)]
            others = [c for c in block if c not in ring]
            rng.shuffle(others)
            sign = 1 if rng.random() < 0.5 else -1   # everybody else faces the neighbour nearest to the ring (tails), or the farthest (a bare cycle)
            for c in others[:N - k]:
                best = min(DXY, key=lambda d: (sign * min(abs(c[0] + DXY[d][0] - r[0]) + abs(c[1] + DXY[d][1] - r[1]) for r in ring), d))
                cells.append(c)
                dirs.append(best)
        else:
            idx = rng.permutation(len(block))[:N]
            cells = [block[i] for i in idx]
            dirs = [int(d) for d in rng.integers(0, 4, size=N)]
        if len(cells) < N:
            continue
        dirs = [int(rng.integers(0, 4)) if rng.random() < 0.06 else d for d in dirs]
        # who stands where: loaded agents on cells without a standing shelf, everybody else at random
        order = [int(i) for i in rng.permutation(N)]
        loaded = [i for i in order if ac[i]]
        slots = list(range(N))
        good = [s for s in slots if cells[s] in ok_loaded]
        if len(good) < len(loaded):
            continue
        rng.shuffle(good)
        assign = {}
        for i, s in zip(loaded, good):
            assign[i] = s
        left = [s for s in slots if s not in assign.values()]
        rng.shuffle(left)
        for i, s in zip([i for i in order if not ac[i]], left):
            assign[i] = s
        nx_, ny_, nd_ = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        for i, s in assign.items():
            nx_[i], ny_[i], nd_[i] = cells[s][0], cells[s][1], dirs[s]
        return nx_, ny_, nd_
    raise AssertionError("no dense block found")
