#!/usr/bin/env python3
"""A/B of the uint8 image format (RW_OBS_IMAGE_U8) against the float32 IMAGE rows, same box, one process per leg.

    image_u8_ab.py --parent-lib PATH/librware_hip.so [--out FILE] [--reps 3] [--steps 2000] [--warmup 200] [--only NAME ...]

Legs, per configuration, alternating `--reps` times (the figure of a leg is the median of its repetitions):
    a  the PARENT commit's library (built from a `git worktree` of HEAD~1 into a scratch directory; it travels as a .so), float32 IMAGE
    b  this tree's library, float32 IMAGE
    c  this tree's library, uint8 IMAGE
Every leg drives the C-ABI directly (ctypes): a device tape of 64 random action rows, `--warmup` untimed steps, then `--steps` steps
timed with the engine's own events riding on the first / last dispatch (rw_step_tape_device_timed).  `rollout-*`: launches of 64 fused
steps between two recorded events.  Un-profiled.  Prints one table; `spread(a)` is (max - min) / median over the repetitions of leg a —
the noise floor: "engines without the flag are unchanged" is b within spread(a) of a; c is reported as measured."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = {   # every one with observation_type IMAGE and the default layer list
    "small-4ag IMAGE x 16384": ("rware-small-4ag-v1", {}, 16384, False),
    "small-4ag IMAGE x 262144": ("rware-small-4ag-v1", {}, 262144, False),
    "large-16ag sr2 IMAGE x 16384": ("rware-large-16ag-v1", {"sensor_range": 2}, 16384, False),
    "rollout-64: small-4ag IMAGE x 16384": ("rware-small-4ag-v1", {}, 16384, True),
}
RW_OBS_IMAGE_U8 = 8192
RW_OBS_IMAGE = 2


def run_leg(args):
    import numpy as np

    import rware_amd
    from rware_amd import _capi

    env_id, extra, B, rollout = CONFIGS[args.config]
    kw = dict(rware_amd.env_kwargs(env_id), **extra)
    lay = rware_amd.layout_from_params(kw["shelf_columns"], kw.get("shelf_rows", 1), kw["column_height"])
    lib = C.CDLL(os.path.abspath(args.lib))
    vp, i32 = C.c_void_p, C.c_int32
    for name, at in (("rw_create", [C.POINTER(_capi.RwConfig), C.POINTER(vp)]), ("rw_destroy", [vp]), ("rw_reset", [vp, vp, vp]),
                     ("rw_step_device", [vp, vp]), ("rw_step_tape_device", [vp, vp, i32, i32, i32]),
                     ("rw_step_tape_device_timed", [vp, vp, i32, i32, i32, i32, i32]), ("rw_step_many_device", [vp, vp, i32, vp, vp, vp]),
                     ("rw_device_malloc", [vp, C.c_size_t, C.POINTER(vp)]), ("rw_copy_to_device", [vp, vp, vp, C.c_size_t]),
                     ("rw_event_record", [vp, i32]), ("rw_event_elapsed_ms", [vp, i32, i32, C.POINTER(C.c_float)]), ("rw_sync", [vp]),
                     ("rw_get_buffer", [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]), ("rw_get_info", [vp, vp])):
        getattr(lib, name).argtypes = at
    lib.rw_last_error.restype = C.c_char_p
    lib.rw_last_error.argtypes = [vp]
    u8 = args.leg == "c"
    hw = np.ascontiguousarray(lay.highways, dtype=np.uint8)
    goals = np.ascontiguousarray(np.asarray(lay.goals, dtype=np.int32).reshape(-1))
    N, R = kw["n_agents"], kw["sensor_range"]
    cfg = _capi.RwConfig(lib.rw_abi_version(), B, lay.grid_size[0], lay.grid_size[1], N, R, kw["request_queue_size"],
                         int(kw.get("max_inactivity_steps") or 0), int(kw.get("max_steps") or 0), kw["reward_type"].value, 0, 1,
                         len(lay.goals), 0, 0, 0, RW_OBS_IMAGE, 1, 0, (C.c_int32 * 8)(), 0, RW_OBS_IMAGE_U8 if u8 else 0,
                         hw.ctypes.data, goals.ctypes.data, None)
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
    if rollout:
        for _ in range(max(1, args.warmup // K)):
            ck(lib.rw_step_many_device(h, d_tape, K, None, None, None))
        n = max(1, args.steps // K)
        ck(lib.rw_event_record(h, 0))
        for _ in range(n):
            ck(lib.rw_step_many_device(h, d_tape, K, None, None, None))
        ck(lib.rw_event_record(h, 1))
        steps = n * K
    else:
        ck(lib.rw_step_tape_device(h, d_tape, K, 0, args.warmup))
        ck(lib.rw_sync(h))
        ck(lib.rw_step_tape_device_timed(h, d_tape, K, 0, args.steps, 0, 1))
        steps = args.steps
    ck(lib.rw_event_elapsed_ms(h, 0, 1, C.byref(ms)))
    ck(lib.rw_sync(h))
    print(json.dumps({"config": args.config, "leg": args.leg, "us_per_step": 1e3 * ms.value / steps, "steps": steps, "build_kind": info.build_kind,
                      "jit": info.jit, "E": info.envs_per_workgroup, "nt": info.obs_stores_stream, "obs_packed": info.obs_packed,
                      "obs_bytes_per_step": B * N * info.obs_length * (1 if info.obs_packed == 2 else 4)}))
    lib.rw_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--lib")
    ap.add_argument("--config")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    own = os.path.join(ROOT, "robotic-warehouse_amd", "csrc", "librware_hip.so")
    libs = {"a": args.parent_lib, "b": own, "c": own}
    res = {}
    for rep in range(args.reps):
        for cname in CONFIGS:
            if args.only and not any(o in cname for o in args.only):
                continue
            for leg in "abc":
                if not libs[leg]:
                    continue
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--lib", libs[leg], "--config", cname, "--steps",
                                    str(args.steps), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=300)
                if p.returncode != 0:   # a leg that fails ends the run: nothing more is started on the device
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit(f"leg {leg} of {cname} failed (rc {p.returncode})")
                r = json.loads(p.stdout.strip().splitlines()[-1])
                res.setdefault((cname, leg), []).append(r)
                print(f"rep {rep} {cname} {leg}: {r['us_per_step']:.3f} us  kind {r['build_kind']} jit {r['jit']} E {r['E']} nt {r['nt']}", flush=True)
    lines = ["# us per step, median of %d alternations (all repetitions in brackets); %d timed steps after %d warm-up steps, un-profiled" %
             (args.reps, args.steps, args.warmup),
             "# a = parent commit's library, float32 IMAGE | b = this tree, float32 IMAGE | c = this tree, uint8 IMAGE (RW_OBS_IMAGE_U8)",
             "# config | a | b | c | spread(a) | b/a | b within spread(a) of a? | c/a | c faster than a by more than spread(a)?"]
    for cname in CONFIGS:
        if (cname, "b") not in res:
            continue
        med = {l: statistics.median(r["us_per_step"] for r in res[(cname, l)]) for l in "abc" if (cname, l) in res}
        allv = {l: "[" + " ".join(f"{r['us_per_step']:.2f}" for r in res[(cname, l)]) + "]" for l in med}
        cell = lambda l: f"{med[l]:.3f} {allv[l]}" if l in med else "-"
        if "a" in med:
            va = [r["us_per_step"] for r in res[(cname, "a")]]
            spread = (max(va) - min(va)) / med["a"]
            tail = (f"{100 * spread:.1f} % | {med['b'] / med['a']:.3f} | {'yes' if abs(med['b'] - med['a']) <= spread * med['a'] else 'NO'} | "
                    f"{med['c'] / med['a']:.3f} | {'yes' if med['c'] < med['a'] * (1 - spread) else 'NO'}")
        else:
            tail = "- | - | - | - | -"
        kinds = " ".join(f"{l}:kind{res[(cname, l)][0]['build_kind']}/jit{res[(cname, l)][0]['jit']}/E{res[(cname, l)][0]['E']}" for l in med)
        lines.append(f"{cname} | {cell('a')} | {cell('b')} | {cell('c')} | {tail}   ({kinds})")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
