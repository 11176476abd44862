#!/usr/bin/env python3
"""Same-box A/B of this tree's library against the PARENT commit's: one harness, the experiments as data.

    ab.py EXPERIMENT --parent-lib PATH/librware_hip.so [--out FILE] [--reps N] [--only NAME ...] [--steps N --warmup N]

The parent's library comes from a `git worktree` of HEAD~1 built into a scratch directory (it travels as a .so).  Every leg of an
experiment is a child process (`ab.py --leg <json>`, one at a time) that drives the C-ABI directly through rware_amd._capi's description
of it (declare + make_config; options by keyword, buffer kinds through _capi.BUF; a parent library is handed its own rw_abi_version()):
a device tape of 64 random action rows, warm-up steps, then the timed steps, un-profiled, back to back.  Modes:
    step         the engine's own events ride on the first / last dispatch (rw_step_tape_device_timed)
    rollout      launches of <tape rows> fused steps (rw_step_many_device) between two recorded events
    step+unpack  every step followed by rw_unpack_obs of the whole batch, recorded events around the pairs: the host side issues two
                 calls per step (at small batches that leg may be bound by the host)
The legs of a configuration alternate `--reps` times (some experiments drop a first alternation: it warms the run-time builds' disk
cache); the figure of a leg is the median of its repetitions, [min .. max] beside it.  Acceptance is ONE rule, verdict(): own / parent
on the medians has to lie inside what single parent runs give against each other."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OWN_LIBRARY = os.path.join(ROOT, "robotic-warehouse_amd", "csrc", "librware_hip.so")
SMALL4, LARGE16 = "rware-small-4ag-v1", "rware-large-16ag-v1"
IDENTITY = ("build_kind", "jit", "E", "nt", "stats", "obs_packed", "bytes", "steps")   # equal on two legs: the same engine, the same launches


def config(env_id, envs, steps=2000, warmup=200, mode="step", **more):
    return dict(env_id=env_id, envs=envs, steps=steps, warmup=warmup, mode=mode, **more)


def legs(*rows):
    """(name, "parent" | "own", options, description[, mode]) rows -> {name: leg}"""
    return {r[0]: dict(lib=r[1], options=r[2], text=r[3], mode=r[4] if len(r) > 4 else None) for r in rows}


THREE = {   # per-step at one and at sixteen rounds of workgroups, and the fused rollout: what a change to the step kernels can move
    "small-4ag x 16384": config(SMALL4, 16384, 4000, 400),
    "small-4ag x 262144": config(SMALL4, 262144, 600, 100),
    "rollout-64: small-4ag x 16384": config(SMALL4, 16384, 2560, 256, "rollout"),
}
HEADLINE = {"small-4ag x 16384": config(SMALL4, 16384)}
PARENT_OWN_PARENT = legs(("a", "parent", {}, "parent, no flags"), ("b", "own", {}, "this,   no flags"), ("a2", "parent", {}, "parent, no flags (again)"))
IMAGE = dict(observation_type=2)
# name -> configs, legs, compare: (own leg, parent legs) pairs judged by verdict(), reps, drop_first, extras: legs that time something
# other than steps — (name, spec of a function of this file)
EXPERIMENTS = {
    # the check every refactor needs: nothing the compiler reads changed, so own / parent has to come out inside the parent's own spread
    "baseline": dict(configs=THREE, legs=PARENT_OWN_PARENT, compare=[("b", ("a", "a2"))], reps=5),
    # the valid-action masks (RW_ACTION_MASK_ON) and the dead code they add to the builds that share RW_STATS_BUILD: a / b the
    # ahead-of-time builds (the same ISA); c .. f run-time builds with RW_STATS_BUILD (what the added dead code costs); g the flag itself
    "action_mask": dict(configs=THREE, reps=5, drop_first=True, compare=[("b", ("a",)), ("d", ("c",)), ("f", ("e",))], legs=legs(
        ("a", "parent", {}, "parent, no flags"), ("b", "own", {}, "this,   no flags"),
        ("c", "parent", {"stats": True}, "parent, stats=True"), ("d", "own", {"stats": True}, "this,   stats=True"),
        ("e", "parent", {"episodes": True}, "parent, episode_stats=True"), ("f", "own", {"episodes": True}, "this,   episode_stats=True"),
        ("g", "own", {"action_mask": True}, "this,   action_mask=True"))),
    # time-limit truncation (RW_TIME_LIMIT_TRUNCATES): a, a2 the parent twice (the parent-against-parent spread the no-flag ratio is
    # judged by); b the ahead-of-time builds (the same ISA, two more kernel arguments); c / d what the added dead code costs the
    # run-time builds; e the flag itself (two byte streams instead of one)
    "time_limit": dict(configs=THREE, reps=5, drop_first=True, compare=[("b", ("a", "a2")), ("d", ("c",))], legs=legs(
        ("a", "parent", {}, "parent, no flags"), ("b", "own", {}, "this,   no flags"), ("a2", "parent", {}, "parent, no flags (again)"),
        ("c", "parent", {"action_mask": True}, "parent, action_mask=True"), ("d", "own", {"action_mask": True}, "this,   action_mask=True"),
        ("e", "own", {"time_limit_truncates": True}, "this,   time_limit_truncates=True"))),
    # the packed observation format (RW_OBS_PACKED) against the float32 rows
    "packed_obs": dict(reps=3, compare=[("b", ("a",)), ("c", ("a",))], configs={
        "small-4ag x 16384 (headline)": config(SMALL4, 16384), "small-4ag x 32768": config(SMALL4, 32768),
        "small-4ag x 262144": config(SMALL4, 262144), "small-10ag x 16384": config("rware-small-10ag-v1", 16384),
        "large-16ag x 16384": config(LARGE16, 16384),
        "config 5 shard: large-16ag sr2 x 16384": config(LARGE16, 16384, sensor_range=2),
        "rollout-64: small-4ag x 16384": config(SMALL4, 16384, mode="rollout")}, legs=legs(
        ("a", "parent", {}, "parent, float32"), ("b", "own", {}, "this,   float32"), ("c", "own", {"obs_packed": True}, "this,   packed"),
        ("d", "own", {"obs_packed": True}, "this,   packed + rw_unpack_obs of the batch", "step+unpack"))),
    # the uint8 image format (RW_OBS_IMAGE_U8) against the float32 IMAGE rows; every configuration with the default layer list
    "image_u8": dict(reps=3, compare=[("b", ("a",)), ("c", ("a",))], configs={
        "small-4ag IMAGE x 16384": config(SMALL4, 16384, **IMAGE), "small-4ag IMAGE x 262144": config(SMALL4, 262144, **IMAGE),
        "large-16ag sr2 IMAGE x 16384": config(LARGE16, 16384, sensor_range=2, **IMAGE),
        "rollout-64: small-4ag IMAGE x 16384": config(SMALL4, 16384, mode="rollout", **IMAGE)}, legs=legs(
        ("a", "parent", {}, "parent, float32 IMAGE"), ("b", "own", {}, "this,   float32 IMAGE"),
        ("c", "own", {"obs_image_u8": True}, "this,   uint8 IMAGE"))),
    # what the device path of reset() costs and saves (rw_reset_device), and that the per-step time did not move
    "reset_device": dict(configs=HEADLINE, legs=PARENT_OWN_PARENT, compare=[("b", ("a", "a2"))], reps=5,
                         extras=[(f"reset wall time: {B} envs", dict(fn="reset", env_id=SMALL4, envs=B)) for B in (16384, 262144)]),
    # what the device form of get_global_image costs and saves (rw_global_image), and that the per-step time did not move
    "global_image": dict(configs=HEADLINE, legs=PARENT_OWN_PARENT, compare=[("b", ("a", "a2"))], reps=5,
                         extras=[(f"global image: {e.replace('rware-', '').replace('-v1', '')}, {B} envs", dict(fn="image", env_id=e, envs=B))
                                 for e, B in ((SMALL4, 16384), (SMALL4, 262144), (LARGE16, 16384))]),
}
# Experiments added since the seven above, in a table of their own; the command line takes the names of both
MORE_EXPERIMENTS = {
    # what the indexed restore costs and saves (rw_snapshot_restore_indexed), and that the per-step time did not move
    "restore_indexed": dict(configs=THREE, legs=PARENT_OWN_PARENT, compare=[("b", ("a", "a2"))], reps=5,
                            extras=[(f"indexed restore: {e.replace('rware-', '').replace('-v1', '')}, {B} envs", dict(fn="restore", env_id=e, envs=B))
                                    for e, B in ((SMALL4, 16384), (SMALL4, 262144), (LARGE16, 16384))]),
}
NEEDS = {"step": ("rw_step_tape_device", "rw_step_tape_device_timed"), "rollout": ("rw_step_many_device", "rw_event_record"),
         "step+unpack": ("rw_step_tape_device", "rw_step_device", "rw_unpack_obs", "rw_get_buffer", "rw_event_record")}


def step_leg(spec):
    """One engine on spec["lib"], spec["mode"] timed; prints one JSON line."""
    import ctypes as C

    import numpy as np

    sys.path.insert(0, ROOT)
    import rware_amd
    from rware_amd import _capi

    env_kw = {k: spec[k] for k in ("sensor_range", "observation_type") if k in spec}
    kw = dict(rware_amd.env_kwargs(spec["env_id"]), **env_kw)
    B, N, K, mode, steps, warmup = spec["envs"], kw["n_agents"], spec.get("tape", 64), spec["mode"], spec["steps"], spec["warmup"]
    lib = C.CDLL(os.path.abspath(spec["lib"]))
    needs = ("rw_abi_version", "rw_create", "rw_destroy", "rw_last_error", "rw_get_info", "rw_reset", "rw_device_malloc", "rw_copy_to_device",
             "rw_event_elapsed_ms", "rw_sync", "rw_read") + NEEDS[mode]
    missing = _capi.declare(lib, needs)
    if missing:
        raise SystemExit(f"{spec['lib']} lacks {', '.join(missing)}, which mode {mode!r} needs")
    cfg = _capi.make_config(
        abi_version=lib.rw_abi_version(), num_envs=B, layout=rware_amd.layout_from_params(kw["shelf_columns"], kw.get("shelf_rows", 1), kw["column_height"]),
        n_agents=N, sensor_range=kw["sensor_range"], request_queue_size=kw["request_queue_size"], max_inactivity_steps=kw.get("max_inactivity_steps"),
        max_steps=kw.get("max_steps"), reward_type=kw["reward_type"].value, observation_type=kw.get("observation_type", 1), **spec.get("options", {}))
    h = C.c_void_p()

    def ck(rc):
        if rc != 0:
            raise RuntimeError(f"rc {rc}: {(lib.rw_last_error(h) or lib.rw_last_error(None) or b'').decode()}")
    ck(lib.rw_create(C.byref(cfg), C.byref(h)))
    info = _capi.RwInfo()
    ck(lib.rw_get_info(h, C.byref(info)))
    seeds = np.uint64(7) + np.arange(B, dtype=np.uint64)
    ck(lib.rw_reset(h, seeds.ctypes.data, None))
    tape = np.random.default_rng(0).choice(5, size=(K, B, N), p=[.1, .5, .15, .15, .1]).astype(np.int32)
    d_tape = C.c_void_p()
    ck(lib.rw_device_malloc(h, tape.nbytes, C.byref(d_tape)))
    ck(lib.rw_copy_to_device(h, d_tape, tape.ctypes.data, tape.nbytes))
    if mode == "rollout":
        for _ in range(max(1, warmup // K)):
            ck(lib.rw_step_many_device(h, d_tape, K, None, None, None))
        steps = max(1, steps // K) * K
        ck(lib.rw_event_record(h, 0))
        for _ in range(steps // K):
            ck(lib.rw_step_many_device(h, d_tape, K, None, None, None))
        ck(lib.rw_event_record(h, 1))
    elif mode == "step+unpack":
        d_out, d_packed, nbytes = C.c_void_p(), C.c_void_p(), C.c_size_t()
        ck(lib.rw_device_malloc(h, B * N * info.obs_length * 4, C.byref(d_out)))
        ck(lib.rw_get_buffer(h, _capi.BUF["obs_packed"], C.byref(d_packed), C.byref(nbytes)))
        ck(lib.rw_step_tape_device(h, d_tape, K, 0, warmup))
        ck(lib.rw_unpack_obs(h, d_packed, d_out, B * N))
        ck(lib.rw_sync(h))
        step, unpack, row = lib.rw_step_device, lib.rw_unpack_obs, tape[0].nbytes
        ck(lib.rw_event_record(h, 0))
        for k in range(steps):   # (unchecked inside the timed loop; rw_sync below reports what went wrong)
            step(h, d_tape.value + (k % K) * row)
            unpack(h, d_packed, d_out, B * N)
        ck(lib.rw_event_record(h, 1))
    else:
        ck(lib.rw_step_tape_device(h, d_tape, K, 0, warmup))
        ck(lib.rw_sync(h))
        ck(lib.rw_step_tape_device_timed(h, d_tape, K, 0, steps, 0, 1))
    ck(lib.rw_sync(h))
    ms = C.c_float()
    ck(lib.rw_event_elapsed_ms(h, 0, 1, C.byref(ms)))
    env_steps = np.empty(B, np.int32)
    ck(lib.rw_read(h, _capi.BUF["steps"], env_steps.ctypes.data, env_steps.nbytes))
    print(json.dumps({"us_per_step": 1e3 * ms.value / steps, "steps": steps, "build_kind": info.build_kind, "jit": info.jit,
                      "E": info.envs_per_workgroup, "nt": info.obs_stores_stream, "stats": info.stats, "obs_packed": info.obs_packed,
                      "bytes": info.engine_bytes_per_env_step, "abi": lib.rw_abi_version(), "env0_steps": int(env_steps[0])}))
    lib.rw_destroy(h)


def reset_leg(spec):
    """Reset of every second env with per-env seeds on ONE output="torch" env, host wall time from the call to the return of env.sync():
      host    env.reset(seed=<numpy uint64 (B,)>, mask=<numpy bool (B,)>)   — rw_reset: RNG buffer to the host and back, three synchronisations
      device  env.reset(seed=<int64 CUDA tensor>, mask=<bool CUDA tensor>)  — rw_reset_device: mask copy + seed kernel + reset launch, enqueued
    and, for the device form, the time to the return of reset() itself (the enqueue).  Both forms are warmed, then alternate `reps` times."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import rware_amd

    B = spec["envs"]
    env = rware_amd.WarehouseVecEnv(B, output="torch", **rware_amd.env_kwargs(spec["env_id"]))
    rng = np.random.default_rng(0)
    mask = np.arange(B) % 2 == 0
    mask_t = torch.from_numpy(mask).cuda()
    env.reset(seed=1)
    env.sync()

    def host():
        seeds = rng.integers(0, 2**63, size=B, dtype=np.int64).astype(np.uint64)
        t0 = time.perf_counter()
        env.reset(seed=seeds, mask=mask)
        env.sync()
        return time.perf_counter() - t0, None

    def device():
        seeds_t = torch.from_numpy(rng.integers(0, 2**63, size=B, dtype=np.int64)).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.reset(seed=seeds_t, mask=mask_t)
        t1 = time.perf_counter()
        env.sync()
        return time.perf_counter() - t0, t1 - t0

    for _ in range(3):
        host(), device()
    out = {"host": [], "device": [], "device_enqueue": []}
    for _ in range(spec["reps"]):
        out["host"].append(host()[0])
        total, enqueue = device()
        out["device"].append(total)
        out["device_enqueue"].append(enqueue)
    print(json.dumps({k: [1e6 * x for x in v] for k, v in out.items()}))
    env.close()


LAYERS = [0, 1, 2, 5, 6]   # SHELVES, REQUESTS, AGENTS, GOALS, ACCESSIBLE


def image_leg(spec):
    """The global image of one output="torch" env, 20 random steps into its episodes:
    (a) host    env.get_global_image(layers, recompute=True): get_state() — the int32 grid and the agent arrays to the host — then numpy;
                host wall time, call to result.
    (b) device  env.global_image_device(layers, dtype=...) float32 and uint8: host wall time from the call to the return of env.sync()
                behind it, and to the return of the call itself (the enqueue).  (a) and (b) are warmed, then alternate `reps` times.  The
                first device call behind the host form — the first launch after tens of milliseconds in which the process enqueued
                nothing — is timed apart (its enqueue alone): what a loop that calls every step does not pay.
    (c) kernel  100 calls captured into one HIP graph on a stream of the env's own and replayed five times between two events: us per
                launch (median of the five), against rw_debug_store_floor — a launch that only stores — of a second engine of the same
                configuration whose observation buffer has the byte count of the float32 image (its batch is chosen for that; the
                figure is scaled by the remaining ratio of the two byte counts)."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import rware_amd

    B, kw = spec["envs"], rware_amd.env_kwargs(spec["env_id"])
    env = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
    eng = env.engines[0]
    rng = np.random.default_rng(0)
    env.reset(seed=1)
    for _ in range(20):
        env.step(torch.from_numpy(rng.choice(5, size=(B, env.n_agents), p=[.1, .5, .15, .15, .1]).astype(np.int32)).cuda())
    env.sync()

    def host():
        t0 = time.perf_counter()
        img = env.get_global_image(LAYERS, recompute=True)
        return time.perf_counter() - t0, None, img

    def device(dtype):
        t0 = time.perf_counter()
        img = env.global_image_device(LAYERS, dtype=dtype)
        t1 = time.perf_counter()
        env.sync()
        return time.perf_counter() - t0, t1 - t0, img

    for _ in range(3):
        want = host()[2]
        got32, got8 = device("float32")[2], device("uint8")[2]
    assert np.array_equal(got32.cpu().numpy(), want) and np.array_equal(got8.cpu().numpy(), want.astype(np.uint8))
    out = {"host": [], "f32_first": [], "f32": [], "f32_enq": [], "u8": [], "u8_enq": []}
    for _ in range(spec["reps"] if B <= 65536 else max(5, spec["reps"] // 5)):   # (the host form takes seconds at 262144 envs)
        out["host"].append(host()[0])
        out["f32_first"].append(device("float32")[1])   # the first launch behind tens of ms of host work: its enqueue alone, kept apart
        for key, dtype in (("f32", "float32"), ("u8", "uint8")):
            total, enq, _ = device(dtype)
            out[key].append(total)
            out[key + "_enq"].append(enq)
    res = {k: [1e6 * x for x in v] for k, v in out.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    eng.set_stream(s.cuda_stream)
    n = 100
    for key, dtype, t in (("f32", np.float32, got32), ("u8", np.uint8, got8)):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            s.synchronize()
            with torch.cuda.graph(g, stream=s):
                for _ in range(n):
                    eng.global_image(LAYERS, t.data_ptr(), None, dtype)
            g.replay()
            s.synchronize()
            times = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                g.replay()
                e1.record(s)
                s.synchronize()
                times.append(1e3 * e0.elapsed_time(e1) / n)
        res[key + "_kernel_us"] = statistics.median(times)
        res[key + "_bytes"] = t.numel() * t.element_size()
    assert np.array_equal(got32.cpu().numpy(), want)
    obs_bytes_per_env = env.n_agents * env.obs_length * 4   # the store-only launch: a float32 observation buffer as large as the float32 image
    Bf = max(64, int(round(res["f32_bytes"] / obs_bytes_per_env / 64.0)) * 64)
    floor_env = rware_amd.WarehouseVecEnv(Bf, **kw)
    floor_env.reset(seed=1)
    floor_env.sync()
    res["floor_bytes"] = Bf * obs_bytes_per_env
    res["floor_us_same_bytes"] = 1e3 * floor_env.engines[0].debug_store_floor(200) * res["f32_bytes"] / res["floor_bytes"]
    floor_env.close()
    env.close()
    print(json.dumps(res))


def restore_leg(spec):
    """"Every second env takes the state of a random slot" on one output="torch" env, 20 random steps behind the snapshot:
    (a) host    get_state(), a numpy fancy index, set_state() — the only way without the entry point; host wall time, call to the return of
                env.sync().
    (b) device  env.restore(token, index=<int32 CUDA tensor>): host wall time from the call to the return of env.sync() behind it, and to the
                return of the call itself (the enqueue).  (a) and (b) are warmed, then alternate `reps` times.
    (c) kernel  with the identity index, 50 calls each captured into one HIP graph on a stream of the env's own and replayed five times
                between two events (us per call, median of the five): restore_indexed (gather + observation launch), refresh_obs (the
                observation launch alone), snapshot(into=token) (rw_snapshot_save: the device-to-device copies of the same bytes and
                nothing else).  The gather alone is the first minus the second."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import rware_amd

    B, kw = spec["envs"], rware_amd.env_kwargs(spec["env_id"])
    env = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
    eng = env.engines[0]
    rng = np.random.default_rng(0)
    play = lambda n: [env.step(torch.from_numpy(rng.choice(5, size=(B, env.n_agents), p=[.1, .5, .15, .15, .1]).astype(np.int32)).cuda()) for _ in range(n)]
    env.reset(seed=1)
    play(20)
    token = env.snapshot()
    saved = env.get_state()
    play(20)
    env.sync()
    index = np.where(np.arange(B) % 2 == 0, rng.integers(0, B, size=B), -1).astype(np.int32)
    hit, src = index >= 0, index[index >= 0]
    index_t = torch.from_numpy(index).cuda()
    torch.cuda.synchronize()

    def host():
        t0 = time.perf_counter()
        st = env.get_state()
        for k in st:
            st[k][hit] = saved[k][src]
        env.set_state(**st)
        env.sync()
        return time.perf_counter() - t0, None

    def device():
        t0 = time.perf_counter()
        env.restore(token, index=index_t)
        t1 = time.perf_counter()
        env.sync()
        return time.perf_counter() - t0, t1 - t0

    for _ in range(2):
        host(), device()
    out = {"host": [], "device": [], "device_enq": []}
    for _ in range(spec["reps"] if B <= 65536 else max(5, spec["reps"] // 5)):   # (the host form takes seconds at 262144 envs)
        out["host"].append(host()[0])
        total, enq = device()
        out["device"].append(total)
        out["device_enq"].append(enq)
    want = env.get_state()                       # the host form and the device form have to leave the same state
    play(3)
    env.restore(token, index=index_t)
    env.sync()
    got = env.get_state()
    assert all(np.array_equal(got[k][hit], want[k][hit]) for k in want)
    res = {k: [1e6 * x for x in v] for k, v in out.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    eng.set_stream(s.cuda_stream)
    ident = torch.arange(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = 50
    calls = {"indexed": lambda: eng.restore_indexed(token[0], ident.data_ptr()), "obs": eng.refresh_obs, "copies": lambda: eng.snapshot(into=token[0]),
             "restore": lambda: eng.restore(token[0])}
    for key, call in calls.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            s.synchronize()
            with torch.cuda.graph(g, stream=s):
                for _ in range(n):
                    call()
            g.replay()
            s.synchronize()
            times = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                g.replay()
                e1.record(s)
                s.synchronize()
                times.append(1e3 * e0.elapsed_time(e1) / n)
        res[key + "_us"] = statistics.median(times)
    res["state_bytes"] = B * (env.n_agents * 4 + 8 + 4 * eng.Q + 48 + env.n_agents * 4 + eng.H * eng.W * (2 if eng.S > 255 else 1))
    env.free_snapshot(token)
    env.close()
    print(json.dumps(res))


LEG_FUNCTIONS = {"step": step_leg, "reset": reset_leg, "image": image_leg, "restore": restore_leg}
med = statistics.median
spread = lambda v: (max(v) - min(v)) / med(v)
cell = lambda v: f"{med(v):.1f} ({100 * spread(v):.0f} %)"


def extra_line(fn, r):
    """One report line of a reset / image / restore leg: us, median ((max - min) / median)."""
    if fn == "restore":
        gather = r["indexed_us"] - r["obs_us"]
        return (f"host get_state() + numpy index + set_state() {cell(r['host'])} | device restore(token, index=tensor), call to sync() {cell(r['device'])}, "
                f"call alone {cell(r['device_enq'])} | host / device {med(r['host']) / med(r['device']):.0f} | identity index, replayed from a graph: "
                f"gather + observation launch {r['indexed_us']:.1f} us, observation launch alone {r['obs_us']:.1f} us, gather alone (the difference) "
                f"{gather:.1f} us ({r['state_bytes'] / 1e6:.1f} MB: {2 * r['state_bytes'] / max(gather, 1e-3) / 1e3:.0f} GB/s read + written) | the same "
                f"bytes as device-to-device copies (rw_snapshot_save) {r['copies_us']:.1f} us, rw_snapshot_restore (copies + observation launch) "
                f"{r['restore_us']:.1f} us | gather / copies {gather / r['copies_us']:.2f}")
    if fn == "reset":
        return (f"host reset(seed=array, mask=array) {cell(r['host'])} | device reset(seed=tensor, mask=tensor) {cell(r['device'])} | device, enqueue alone "
                f"{cell(r['device_enqueue'])} | host / device {med(r['host']) / med(r['device']):.1f}")
    gbs = lambda key: f"{r[key + '_kernel_us']:.1f} us ({r[key + '_bytes'] / r[key + '_kernel_us'] / 1e3:.0f} GB/s)"
    return (f"host get_global_image(recompute=True) {cell(r['host'])} | device float32, call to sync() {cell(r['f32'])}, call alone {cell(r['f32_enq'])} | "
            f"device uint8 {cell(r['u8'])}, call alone {cell(r['u8_enq'])} | host / device {med(r['host']) / med(r['f32']):.1f} (float32) "
            f"{med(r['host']) / med(r['u8']):.1f} (uint8) | first call behind the host form, call alone {cell(r['f32_first'])} | kernel alone, "
            f"{r['f32_bytes'] / 1e6:.1f} MB float32: {gbs('f32')}, uint8 {gbs('u8')}, store-only of the same bytes {r['floor_us_same_bytes']:.1f} us "
            f"(measured on {r['floor_bytes'] / 1e6:.1f} MB): kernel / store-only {r['f32_kernel_us'] / r['floor_us_same_bytes']:.2f}")


def verdict(own_runs, parent_runs):
    """The acceptance rule: ratio = median(own) / median(all parent runs) is "inside" iff min(p) / max(p) <= ratio <= max(p) / min(p)
    over the single parent runs p — what the parent gives against itself on this box.  Fewer than two parent runs: "no spread"."""
    ratio = med(own_runs) / med(parent_runs)
    if len(parent_runs) < 2:
        return dict(ratio=ratio, word="no spread", text=f"{ratio:.4f}; {len(parent_runs)} parent run: no spread to judge it by")
    lo, hi = min(parent_runs) / max(parent_runs), max(parent_runs) / min(parent_runs)
    word = "inside" if lo <= ratio <= hi else "OUTSIDE"
    return dict(ratio=ratio, lo=lo, hi=hi, word=word, text=f"{ratio:.4f}; single parent runs against each other {lo:.4f} .. {hi:.4f} "
                f"((max - min) / median {100 * spread(parent_runs):.2f} %): {word} the spread")


def child(spec):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", json.dumps(spec)], capture_output=True, text=True, timeout=300)
    if p.returncode != 0:   # a leg that fails ends the run: nothing more is started on the device
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"leg {spec} failed (rc {p.returncode})")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("experiment", nargs="?", choices=sorted({**EXPERIMENTS, **MORE_EXPERIMENTS}))
    ap.add_argument("--leg", help="(internal) run one leg, a JSON spec, in this process")
    ap.add_argument("--parent-lib")
    ap.add_argument("--own-lib", default=OWN_LIBRARY)
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int)
    ap.add_argument("--extra-reps", type=int, default=30, help="alternations inside a reset / image leg")
    ap.add_argument("--only", nargs="*", help="configurations / extra legs whose name contains one of these")
    for name in ("steps", "warmup", "envs", "tape"):
        ap.add_argument("--" + name, type=int, help="override for every configuration")
    args = ap.parse_args()
    if args.leg:
        spec = json.loads(args.leg)
        return LEG_FUNCTIONS[spec.get("fn", "step")](spec)
    if not args.experiment or not args.parent_lib:
        ap.error("an experiment and --parent-lib are required")
    exp = {**EXPERIMENTS, **MORE_EXPERIMENTS}[args.experiment]
    libs = {"parent": args.parent_lib, "own": args.own_lib}
    reps, drop = args.reps or exp["reps"], 1 if exp.get("drop_first") else 0
    wanted = lambda name: not args.only or any(o in name for o in args.only)
    override = {k: getattr(args, k) for k in ("steps", "warmup", "envs", "tape") if getattr(args, k) is not None}
    lines = []
    for name, spec in exp.get("extras", ()):
        if wanted(name):
            lines.append(f"{name}: " + extra_line(spec["fn"], child(dict(spec, reps=args.extra_reps))))
            print(lines[-1], flush=True)
    res = {}
    for rep in range(reps + drop):   # (with drop_first, repetition 0 warms the run-time builds' disk cache and is dropped)
        for cname, conf in exp["configs"].items():
            for lname, leg in exp["legs"].items():
                if not wanted(cname) or (leg["mode"] and conf["mode"] != "step"):
                    continue
                r = child(dict(conf, **override, lib=libs[leg["lib"]], options=leg["options"], mode=leg["mode"] or conf["mode"]))
                if rep >= drop:
                    res.setdefault((cname, lname), []).append(r)
                print(f"rep {rep} {cname} leg {lname}: {r['us_per_step']:.3f} us   " + " ".join(f"{k} {r[k]}" for k in IDENTITY), flush=True)
    lines.append(f"# {args.experiment}: us per step, median of {reps} alternations [min .. max]" + (", one warm-up alternation dropped" if drop else "") +
                 "; un-profiled; then what both legs of a pair must agree on")
    for cname in exp["configs"]:
        runs = {l: [r["us_per_step"] for r in res[(cname, l)]] for l in exp["legs"] if (cname, l) in res}
        if not runs:
            continue
        lines.append(cname)
        for l, v in runs.items():
            r0 = res[(cname, l)][0]
            lines.append(f"  {l:2s} {exp['legs'][l]['text']:42s} {med(v):8.3f} [{min(v):.3f} .. {max(v):.3f}]   " + " ".join(f"{k} {r0[k]}" for k in IDENTITY))
        for own, parents in exp["compare"]:
            if own in runs and all(p in runs for p in parents):
                lines.append(f"  {own} / {' + '.join(parents)}: " + verdict(runs[own], [x for p in parents for x in runs[p]])["text"])
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
