"""The fixtures of tests/golden/wide/ (warehouses of 65 .. 127 agents, recorded from the unmodified reference by
tests/golden/wide/generate_wide.py): loading them in the form golden_util.replay takes, and the one question both the generator and
the tests ask of a trace — does a committed chain of movers cross agent index 64, the boundary between the two agents a lane of the
step kernel's wavefront owns.  Plain numpy; used on the CPU and on the GPU box alike (no reference, no oracle)."""
import os

import numpy as np

import pins

WIDE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide")
TRACES = ("tiny-65ag", "small-127ag-twostage", "medium-96ag-msg1-global-inact", "imgdict-medium-100ag-sr2")
SCRIPTED = ("medium-70ag-global-scripted",)   # the delivery-seeking policy instead of random play: GLOBAL rewards get paid
STRADDLE = "collisions-straddle"
SLOT = 64   # agents 0 .. 63 sit in the first slot of their lane, 64 .. 126 in the second


def pack_obs(obs, flattened, lead):
    """float32 observations -> what the fixtures store, generate_observations.pack_observations' formats: FLATTENED rows as two float32
    coordinates + the 0/1 rest bit-packed, images bit-packed (bytes where a layer holds more than 0/1).  `lead`: axes in front of the
    row / image (the packer keeps them)."""
    if flattened:
        rest = obs[..., 2:]
        assert np.isin(rest, (0.0, 1.0)).all()
        return {"obs_xy": obs[..., :2].astype(np.float32), "obs_bits": np.packbits(rest.astype(np.uint8), axis=-1)}
    flat = obs.reshape(obs.shape[:lead] + (-1,))
    assert np.array_equal(flat, flat.astype(np.uint8))
    if flat.max() <= 1:
        return {"img_bits": np.packbits(flat.astype(np.uint8), axis=-1)}
    return {"img_u8": flat.astype(np.uint8)}


def unpack_obs(z, prefix, obs_shape):
    """the float32 observations back: `obs_shape` is one agent's (L,) or (C, h, w)"""
    n = int(np.prod(obs_shape))
    if prefix + "obs_bits" in z:
        bits = np.unpackbits(z[prefix + "obs_bits"], axis=-1, count=n - 2).astype(np.float32)
        return np.concatenate([z[prefix + "obs_xy"].astype(np.float32), bits], axis=-1)
    if prefix + "img_bits" in z:
        flat = np.unpackbits(z[prefix + "img_bits"], axis=-1, count=n)
    else:
        flat = z[prefix + "img_u8"]
    return flat.astype(np.float32).reshape(flat.shape[:-1] + tuple(obs_shape))


def unpack_trace_obs(z):
    """load_npz's `prepare` of a random trace: obs0 / obs (/ features0 / features) unpacked to float32, the packed arrays dropped"""
    z["obs0"] = unpack_obs(z, "init_", z["meta"]["obs_shape"])
    z["obs"] = unpack_obs(z, "", z["meta"]["obs_shape"])
    for k in ("features0", "features"):
        if k in z:
            z[k] = z[k].astype(np.float32)
    for k in [k for k in z if k.endswith(("obs_xy", "obs_bits", "img_bits", "img_u8"))]:
        del z[k]


def load_trace(name):
    """(meta, fields) of a random trace, fields as golden_util.replay reads them (`meta` once more among them)"""
    z = pins.load_npz(WIDE_DIR, name, prepare=unpack_trace_obs)
    return z["meta"], z


def unpack_scenario_obs(z):
    """load_npz's `prepare` of a constructed fixture that stores its observations (no oracle beyond 64 agents)"""
    if "obs_bits" in z:
        z["obs"] = unpack_obs(z, "", z["meta"]["obs_shape"])   # (n, 1 + T, N, L): the injected state, then every step


def load_straddle():
    return pins.load_npz(WIDE_DIR, STRADDLE, prepare=unpack_scenario_obs)


def straddling_chains(x0, y0, x1, y1, W):
    """Committed chains across the slot boundary in ONE env-step: agents' cells before (x0, y0) and after (x1, y1) the step.  A link
    i -> j is committed when i moved onto the cell j stood on (so j moved too); links are joined into chains (and cycles).  Returns the
    list of chains — sorted agent indices — that hold a member below index 64 and one from 64 on."""
    c0, c1 = np.asarray(y0, np.int64) * W + np.asarray(x0, np.int64), np.asarray(y1, np.int64) * W + np.asarray(x1, np.int64)
    at = {int(c): i for i, c in enumerate(c0)}
    parent = list(range(len(c0)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    linked = set()
    for i in range(len(c0)):
        j = at.get(int(c1[i]))
        if c1[i] != c0[i] and j is not None:
            parent[find(i)] = find(j)
            linked.update((i, j))
    groups = {}
    for i in linked:
        groups.setdefault(find(i), []).append(i)
    return [sorted(g) for g in groups.values() if min(g) < SLOT <= max(g)]


def trace_straddles(z, W):
    """[(t, env, chain)] over a random trace: every committed chain across the slot boundary, reset steps left out"""
    out = []
    T, E = z["actions"].shape[:2]
    for t in range(T):
        px, py = (z["init_agent_x"], z["init_agent_y"]) if t == 0 else (z["agent_x"][t - 1], z["agent_y"][t - 1])
        for e in range(E):
            if z["was_reset"][t, e]:
                continue
            out += [(t, e, c) for c in straddling_chains(px[e], py[e], z["agent_x"][t, e], z["agent_y"][t, e], W)]
    return out
