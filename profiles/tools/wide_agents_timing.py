#!/usr/bin/env python3
"""What the generic kernel costs per step at 64, 65, 100 and 127 agents on ONE layout (the medium warehouse, 20 x 16).

    wide_agents_timing.py [--parent-lib PATH/librware_hip.so] [--out FILE] [--reps N] [--envs 4096 16384] [--agents 64 65 100 127]

ab.py's pattern — every leg a child process of its own (`--leg <json>`, one at a time) that drives the C-ABI through rware_amd._capi:
a device tape of 64 random action rows, warm-up steps, then the timed steps, un-profiled, back to back, the engine's own events riding
on the first / last dispatch (rw_step_tape_device_timed); the legs alternate `--reps` times, a figure is the median [min .. max].
Every engine is built with jit="off", so 64 agents run the generic kernel as well (its 64-lane agent phases: one env per wavefront, as
65 and more have it) on the same 4-env workgroups.  No experiment of ab.EXPERIMENTS, no threshold: the yardstick is the parent
library's figure at 64 agents (`--parent-lib`; it refuses more), and what gets recorded is, per agent count, us per step and the
cost per agent-step relative to 64 agents on the same layout and batch."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OWN_LIBRARY = os.path.join(ROOT, "robotic-warehouse_amd", "csrc", "librware_hip.so")
MEDIUM = dict(shelf_columns=5, shelf_rows=2, column_height=8)


def leg(spec):
    import ctypes as C

    import numpy as np

    sys.path.insert(0, ROOT)
    import rware_amd
    from rware_amd import _capi

    B, N, K, steps, warmup = spec["envs"], spec["agents"], 64, spec["steps"], spec["warmup"]
    lib = C.CDLL(os.path.abspath(spec["lib"]))
    missing = _capi.declare(lib, ("rw_abi_version", "rw_create", "rw_destroy", "rw_last_error", "rw_get_info", "rw_reset", "rw_device_malloc",
                                  "rw_copy_to_device", "rw_event_elapsed_ms", "rw_sync", "rw_step_tape_device", "rw_step_tape_device_timed"))
    if missing:
        raise SystemExit(f"{spec['lib']} lacks {', '.join(missing)}")
    cfg = _capi.make_config(abi_version=lib.rw_abi_version(), num_envs=B, layout=rware_amd.layout_from_params(MEDIUM["shelf_columns"], MEDIUM["shelf_rows"], MEDIUM["column_height"]),
                            n_agents=N, sensor_range=1, request_queue_size=N // 2, max_inactivity_steps=None, max_steps=500, reward_type=1,
                            envs_per_workgroup=4, threads_per_workgroup=256, jit="off")
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
    ck(lib.rw_step_tape_device(h, d_tape, K, 0, warmup))
    ck(lib.rw_sync(h))
    ck(lib.rw_step_tape_device_timed(h, d_tape, K, 0, steps, 0, 1))
    ck(lib.rw_sync(h))
    ms = C.c_float()
    ck(lib.rw_event_elapsed_ms(h, 0, 1, C.byref(ms)))
    print(json.dumps({"us_per_step": 1e3 * ms.value / steps, "build_kind": info.build_kind, "E": info.envs_per_workgroup, "lds": info.lds_bytes,
                      "nt": info.obs_stores_stream, "prio": info.wave_priority, "bytes": info.engine_bytes_per_env_step}))
    lib.rw_destroy(h)


def child(spec):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", json.dumps(spec)], capture_output=True, text=True, timeout=300)
    if p.returncode != 0:   # a leg that fails ends the run: nothing more is started on the device
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"leg {spec} failed (rc {p.returncode})")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--leg", help="(internal) run one leg, a JSON spec, in this process")
    ap.add_argument("--parent-lib")
    ap.add_argument("--own-lib", default=OWN_LIBRARY)
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--envs", type=int, nargs="*", default=[4096, 16384])
    ap.add_argument("--agents", type=int, nargs="*", default=[64, 65, 100, 127])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    args = ap.parse_args()
    if args.leg:
        return leg(json.loads(args.leg))
    med = statistics.median
    lines = [f"# wide_agents_timing: the generic kernel (jit off), medium warehouse 20 x 16, 4 envs per 256-thread workgroup, sensor_range 1; us per step, "
             f"median of {args.reps} alternations [min .. max], {args.steps} timed steps behind {args.warmup}; un-profiled"]
    for B in args.envs:
        rows = ([("parent", 64, args.parent_lib)] if args.parent_lib else []) + [("this", n, args.own_lib) for n in args.agents]
        runs = {}
        for rep in range(args.reps):
            for who, n, lib in rows:
                r = child(dict(lib=lib, envs=B, agents=n, steps=args.steps, warmup=args.warmup))
                runs.setdefault((who, n), []).append(r)
                print(f"rep {rep} {B} envs, {who} {n} agents: {r['us_per_step']:.3f} us", flush=True)
        lines.append(f"{B} envs")
        base = {who: med([r["us_per_step"] for r in runs[(who, 64)]]) / 64 for who in ("parent", "this") if (who, 64) in runs}
        for who, n, _ in rows:
            v = [r["us_per_step"] for r in runs[(who, n)]]
            r0 = runs[(who, n)][0]
            per_agent = med(v) / n
            rel = "  ".join(f"per agent-step / {w}'s at 64 agents {per_agent / b:.3f}" for w, b in base.items())
            lines.append(f"  {who:6s} {n:3d} agents  {med(v):9.3f} [{min(v):.3f} .. {max(v):.3f}]  {1e3 * per_agent / B:7.4f} ns per agent-step  {rel}   "
                         f"build_kind {r0['build_kind']} E {r0['E']} lds {r0['lds']} nt {r0['nt']} prio {r0['prio']} bytes {r0['bytes']}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
