#!/usr/bin/env python3
"""A/B of time-limit truncation (RW_TIME_LIMIT_TRUNCATES) and of the dead code it adds to the builds that share RW_STATS_BUILD, against the
PARENT commit's library, same box, one process per leg.

    time_limit_ab.py --parent-lib PATH/librware_hip.so [--out FILE] [--reps 5] [--only NAME ...]

Legs, per configuration, alternating `--reps` times (the figure of a leg is the median of its repetitions, [min .. max] beside it):
    a, a2  parent, no flags (twice: the parent-against-parent spread the no-flag ratio is judged by)
    b      this tree, no flags                                    (the ahead-of-time builds: the same ISA, two more kernel arguments)
    c      parent, RW_ACTION_MASK_ON   d  this tree, RW_ACTION_MASK_ON   (run-time builds with RW_STATS_BUILD: what the added dead code costs)
    e      this tree, RW_TIME_LIMIT_TRUNCATES                     (the flag itself: two byte streams instead of one)
Every leg drives the C-ABI directly (ctypes): a device tape of 64 random action rows, warm-up steps, then the timed steps with the
engine's own events riding on the first / last dispatch (rw_step_tape_device_timed); `rollout-64`: launches of 64 fused steps.
Un-profiled, back to back.  The parent's library comes from a `git worktree` of HEAD~1 built into a scratch directory."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# name -> (env id, envs, timed steps, warm-up steps)
CONFIGS = {
    "small-4ag x 16384": ("rware-small-4ag-v1", 16384, 4000, 400),
    "small-4ag x 262144": ("rware-small-4ag-v1", 262144, 600, 100),
    "rollout-64: small-4ag x 16384": ("rware-small-4ag-v1", 16384, 2560, 256),   # launches of 64 fused steps
}
LEGS = {"a": ("parent", 0), "b": ("own", 0), "a2": ("parent", 0), "c": ("parent", 4096), "d": ("own", 4096), "e": ("own", 16384)}
NAMES = {"a": "parent, no flags", "a2": "parent, no flags (again)", "b": "this,   no flags", "c": "parent, action_mask=True",
         "d": "this,   action_mask=True", "e": "this,   time_limit_truncates=True"}


def run_leg(args):
    import numpy as np

    import rware_amd
    from rware_amd import _capi

    env_id, B, steps, warmup = CONFIGS[args.config]
    kw = rware_amd.env_kwargs(env_id)
    lay = rware_amd.layout_from_params(kw["shelf_columns"], kw.get("shelf_rows", 1), kw["column_height"])
    lib = C.CDLL(os.path.abspath(args.lib))
    vp, i32 = C.c_void_p, C.c_int32
    for name, at in (("rw_create", [C.POINTER(_capi.RwConfig), C.POINTER(vp)]), ("rw_destroy", [vp]), ("rw_reset", [vp, vp, vp]),
                     ("rw_step_tape_device", [vp, vp, i32, i32, i32]), ("rw_step_tape_device_timed", [vp, vp, i32, i32, i32, i32, i32]),
                     ("rw_device_malloc", [vp, C.c_size_t, C.POINTER(vp)]), ("rw_step_many_device", [vp, vp, i32, vp, vp, vp]),
                     ("rw_copy_to_device", [vp, vp, vp, C.c_size_t]), ("rw_event_record", [vp, i32]),
                     ("rw_event_elapsed_ms", [vp, i32, i32, C.POINTER(C.c_float)]), ("rw_sync", [vp]), ("rw_get_info", [vp, vp])):
        getattr(lib, name).argtypes = at
    lib.rw_last_error.restype = C.c_char_p
    lib.rw_last_error.argtypes = [vp]
    hw = np.ascontiguousarray(lay.highways, dtype=np.uint8)
    goals = np.ascontiguousarray(np.asarray(lay.goals, dtype=np.int32).reshape(-1))
    N = kw["n_agents"]
    cfg = _capi.RwConfig(lib.rw_abi_version(), B, lay.grid_size[0], lay.grid_size[1], N, kw["sensor_range"], kw["request_queue_size"],
                         int(kw.get("max_inactivity_steps") or 0), int(kw.get("max_steps") or 0), kw["reward_type"].value, 0, 1,
                         len(lay.goals), 0, 0, 0, 1, 1, 0, (C.c_int32 * 8)(), 0, args.flags, hw.ctypes.data, goals.ctypes.data, None)
    h = vp()

    def ck(rc):
        if rc != 0:
            raise RuntimeError(f"rc {rc}: {(lib.rw_last_error(h) or lib.rw_last_error(None) or b'').decode()}")
    ck(lib.rw_create(C.byref(cfg), C.byref(h)))
    info = _capi.RwInfo()
    ck(lib.rw_get_info(h, C.byref(info)))
    seeds = (np.uint64(7) + np.arange(B, dtype=np.uint64)).astype(np.uint64)
    ck(lib.rw_reset(h, seeds.ctypes.data, None))
    K = 64
    tape = np.random.default_rng(0).choice(5, size=(K, B, N), p=[.1, .5, .15, .15, .1]).astype(np.int32)
    d_tape = vp()
    ck(lib.rw_device_malloc(h, tape.nbytes, C.byref(d_tape)))
    ck(lib.rw_copy_to_device(h, d_tape, tape.ctypes.data, tape.nbytes))
    ms = C.c_float()
    if args.config.startswith("rollout"):
        for _ in range(warmup // K):
            ck(lib.rw_step_many_device(h, d_tape, K, None, None, None))
        ck(lib.rw_event_record(h, 0))
        for _ in range(steps // K):
            ck(lib.rw_step_many_device(h, d_tape, K, None, None, None))
        ck(lib.rw_event_record(h, 1))
    else:
        ck(lib.rw_step_tape_device(h, d_tape, K, 0, warmup))
        ck(lib.rw_sync(h))
        ck(lib.rw_step_tape_device_timed(h, d_tape, K, 0, steps, 0, 1))
    ck(lib.rw_event_elapsed_ms(h, 0, 1, C.byref(ms)))
    ck(lib.rw_sync(h))
    print(json.dumps({"config": args.config, "leg": args.leg, "us_per_step": 1e3 * ms.value / steps, "steps": steps, "build_kind": info.build_kind,
                      "jit": info.jit, "E": info.envs_per_workgroup, "stats": info.stats, "bytes": info.engine_bytes_per_env_step}))
    lib.rw_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--lib")
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--config")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    libs = {"parent": args.parent_lib, "own": os.path.join(ROOT, "robotic-warehouse_amd", "csrc", "librware_hip.so")}
    res = {}
    for rep in range(args.reps + 1):   # (repetition 0 warms the run-time builds' disk cache and is dropped)
        for cname in CONFIGS:
            if args.only and not any(o in cname for o in args.only):
                continue
            for leg, (which, flags) in LEGS.items():
                if not libs[which]:
                    continue
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--lib", libs[which], "--flags", str(flags),
                                    "--config", cname], capture_output=True, text=True, timeout=300)
                if p.returncode != 0:   # a leg that fails ends the run: nothing more is started on the device
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit(f"leg {leg} of {cname} failed (rc {p.returncode})")
                r = json.loads(p.stdout.strip().splitlines()[-1])
                if rep:
                    res.setdefault((cname, leg), []).append(r)
                print(f"rep {rep} {cname} {leg}: {r['us_per_step']:.3f} us  kind {r['build_kind']} jit {r['jit']} E {r['E']} stats {r['stats']}", flush=True)
    lines = [f"# us per step, median of {args.reps} alternations [min .. max], one warm-up alternation dropped; un-profiled, events on the first / last dispatch"]
    for cname in CONFIGS:
        if (cname, "b") not in res:
            continue
        lines.append(f"{cname}   (timed steps {res[(cname, 'b')][0]['steps']})")
        for leg in LEGS:
            if (cname, leg) not in res:
                continue
            v = [r["us_per_step"] for r in res[(cname, leg)]]
            r0 = res[(cname, leg)][0]
            lines.append(f"  {NAMES[leg]:34s} {statistics.median(v):8.3f} [{min(v):.3f} .. {max(v):.3f}]   kind {r0['build_kind']} jit {r0['jit']} E {r0['E']} "
                         f"engine bytes / env-step {r0['bytes']}")
        med = {leg: statistics.median(r["us_per_step"] for r in res[(cname, leg)]) for leg in LEGS if (cname, leg) in res}
        if "a" in med and "a2" in med:   # acceptance: this / parent inside the spread of parent / parent
            lo, hi = sorted((med["a"] / med["a2"], med["a2"] / med["a"]))
            pa = [r["us_per_step"] for leg in ("a", "a2") for r in res[(cname, leg)]]
            ratio = med["b"] / statistics.median(pa)
            ok = min(pa) / max(pa) <= ratio <= max(pa) / min(pa)
            lines.append(f"  no flags, this / parent {ratio:.4f}; parent / parent medians {lo:.4f} .. {hi:.4f}, single runs {min(pa) / max(pa):.4f} .. "
                         f"{max(pa) / min(pa):.4f}: {'inside' if ok else 'OUTSIDE'} the spread")
        if "c" in med and "d" in med:
            lines.append(f"  action_mask=True, this / parent {med['d'] / med['c']:.4f}")
        if "e" in med:
            lines.append(f"  time_limit_truncates=True against this tree without flags {med['e'] - med['b']:+.3f} us, against action_mask=True "
                         f"{med['e'] - med.get('d', float('nan')):+.3f} us")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
