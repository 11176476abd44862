#!/usr/bin/env python3
"""What the device path of reset() costs and saves (rw_reset_device), and that the per-step time did not move.  Same box, un-profiled.

    reset_device_ab.py --parent-lib PATH/librware_hip.so [--out FILE] [--reps 5] [--reset-reps 30] [--steps 2000] [--warmup 200]

(a) reset time, small-4ag x 16384 and x 262144, one process per batch size, one output="torch" env, both forms on that env:
      host    env.reset(seed=<numpy uint64 (B,)>, mask=<numpy bool (B,)>)   — rw_reset: RNG buffer to the host and back, three synchronisations
      device  env.reset(seed=<int64 CUDA tensor>, mask=<bool CUDA tensor>)  — rw_reset_device: mask copy + seed kernel + reset launch, enqueued
    Each is host wall time from the call to the return of env.sync() behind it; for the device form the time to the return of reset()
    itself (the enqueue) is recorded as well.  Both forms are warmed first, then alternate `--reset-reps` times; median and
    (max - min) / median.  Every second env is reset; the seeds differ per repetition.
(b) per-step time, default small-4ag x 16384 engine, this tree's library against the PARENT commit's (built from a `git worktree` of HEAD~1
    into a scratch directory; it travels as a .so): one process per leg driving the C-ABI directly (ctypes), a device tape of 64 random
    action rows, `--warmup` untimed steps, then `--steps` steps timed with the engine's events riding on the first / last dispatch
    (rw_step_tape_device_timed).  Legs a (parent), b (this tree), a' (parent again) alternate `--reps` times; reported: b / a on the medians
    beside the parent-against-parent spread — (max - min) / median over all parent repetitions.  "Unchanged" = |b / a - 1| inside it."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ENV_ID = "rware-small-4ag-v1"


def reset_leg(args):
    import numpy as np
    import torch

    import rware_amd

    B = args.batch
    env = rware_amd.WarehouseVecEnv(B, output="torch", **rware_amd.env_kwargs(ENV_ID))
    rng = np.random.default_rng(0)
    mask = np.arange(B) % 2 == 0
    mask_t = torch.from_numpy(mask).cuda()
    env.reset(seed=1)
    env.sync()

    def host(k):
        seeds = rng.integers(0, 2**63, size=B, dtype=np.int64).astype(np.uint64)
        t0 = time.perf_counter()
        env.reset(seed=seeds, mask=mask)
        env.sync()
        return time.perf_counter() - t0, None

    def device(k):
        seeds_t = torch.from_numpy(rng.integers(0, 2**63, size=B, dtype=np.int64)).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.reset(seed=seeds_t, mask=mask_t)
        t1 = time.perf_counter()
        env.sync()
        return time.perf_counter() - t0, t1 - t0

    for k in range(3):
        host(k), device(k)
    h, d, q = [], [], []
    for k in range(args.reset_reps):
        h.append(host(k)[0])
        total, enq = device(k)
        d.append(total)
        q.append(enq)
    us = lambda v: [1e6 * x for x in v]
    print(json.dumps({"batch": B, "host_us": us(h), "device_us": us(d), "device_enqueue_us": us(q)}))
    env.close()


def step_leg(args):
    import numpy as np

    import rware_amd
    from rware_amd import _capi

    B = 16384
    kw = rware_amd.env_kwargs(ENV_ID)
    lay = rware_amd.layout_from_params(kw["shelf_columns"], kw.get("shelf_rows", 1), kw["column_height"])
    lib = C.CDLL(os.path.abspath(args.lib))
    vp, i32 = C.c_void_p, C.c_int32
    for name, at in (("rw_create", [C.POINTER(_capi.RwConfig), C.POINTER(vp)]), ("rw_destroy", [vp]), ("rw_reset", [vp, vp, vp]),
                     ("rw_step_tape_device", [vp, vp, i32, i32, i32]), ("rw_step_tape_device_timed", [vp, vp, i32, i32, i32, i32, i32]),
                     ("rw_device_malloc", [vp, C.c_size_t, C.POINTER(vp)]), ("rw_copy_to_device", [vp, vp, vp, C.c_size_t]),
                     ("rw_event_elapsed_ms", [vp, i32, i32, C.POINTER(C.c_float)]), ("rw_sync", [vp]), ("rw_get_info", [vp, vp])):
        getattr(lib, name).argtypes = at
    lib.rw_last_error.restype = C.c_char_p
    lib.rw_last_error.argtypes = [vp]
    hw = np.ascontiguousarray(lay.highways, dtype=np.uint8)
    goals = np.ascontiguousarray(np.asarray(lay.goals, dtype=np.int32).reshape(-1))
    N = kw["n_agents"]
    cfg = _capi.RwConfig(lib.rw_abi_version(), B, lay.grid_size[0], lay.grid_size[1], N, kw["sensor_range"], kw["request_queue_size"],
                         int(kw.get("max_inactivity_steps") or 0), int(kw.get("max_steps") or 0), kw["reward_type"].value, 0, 1,
                         len(lay.goals), 0, 0, 0, 1, 1, 0, (C.c_int32 * 8)(), 0, 0, hw.ctypes.data, goals.ctypes.data, None)
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
    ck(lib.rw_step_tape_device(h, d_tape, K, 0, args.warmup))
    ck(lib.rw_sync(h))
    ck(lib.rw_step_tape_device_timed(h, d_tape, K, 0, args.steps, 0, 1))
    ck(lib.rw_sync(h))
    ck(lib.rw_event_elapsed_ms(h, 0, 1, C.byref(ms)))
    print(json.dumps({"us_per_step": 1e3 * ms.value / args.steps, "build_kind": info.build_kind, "jit": info.jit, "E": info.envs_per_workgroup}))
    lib.rw_destroy(h)


def child(extra, timeout=300):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:   # a leg that fails ends the run: nothing more is started on the device
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"leg {extra} failed (rc {p.returncode})")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--lib")
    ap.add_argument("--batch", type=int)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reset-reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    if args.leg == "reset":
        return reset_leg(args)
    if args.leg == "step":
        return step_leg(args)
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    lines = [f"# (a) reset of every second env with per-env seeds, {ENV_ID}: host wall time in us from the call to the return of env.sync(); "
             f"median of {args.reset_reps} alternations ((max - min) / median), after 3 warm-up rounds of both forms; un-profiled",
             "# batch | host: reset(seed=array, mask=array) | device: reset(seed=tensor, mask=tensor) | device, enqueue alone | host / device"]
    for B in (16384, 262144):
        r = child(["--leg", "reset", "--batch", str(B), "--reset-reps", str(args.reset_reps)])
        cell = lambda v: f"{med(v):.1f} ({100 * spread(v):.0f} %)"
        lines.append(f"{B} | {cell(r['host_us'])} | {cell(r['device_us'])} | {cell(r['device_enqueue_us'])} | {med(r['host_us']) / med(r['device_us']):.1f}")
        print(lines[-1], flush=True)
    if args.parent_lib:
        own = os.path.join(ROOT, "robotic-warehouse_amd", "csrc", "librware_hip.so")
        res = {"a": [], "b": []}
        for rep in range(args.reps):
            for leg, lib in (("a", args.parent_lib), ("b", own), ("a", args.parent_lib)):
                r = child(["--leg", "step", "--lib", lib, "--steps", str(args.steps), "--warmup", str(args.warmup)])
                res[leg].append(r)
                print(f"rep {rep} {leg}: {r['us_per_step']:.3f} us  kind {r['build_kind']} jit {r['jit']} E {r['E']}", flush=True)
        va, vb = [r["us_per_step"] for r in res["a"]], [r["us_per_step"] for r in res["b"]]
        ratio, sp = med(vb) / med(va), spread(va)
        lines += ["", f"# (b) us per step, default {ENV_ID} x 16384 engine, {args.steps} timed steps after {args.warmup}; a = parent commit's library "
                      f"({len(va)} runs), b = this tree's ({len(vb)} runs), alternating a b a; un-profiled",
                  "# a median [all] | b median [all] | b / a | parent-against-parent spread (max - min) / median | |b / a - 1| inside it?",
                  f"{med(va):.3f} [{' '.join(f'{x:.3f}' for x in va)}] | {med(vb):.3f} [{' '.join(f'{x:.3f}' for x in vb)}] | {ratio:.4f} | "
                  f"{100 * sp:.2f} % | {'yes' if abs(ratio - 1) <= sp else 'NO'}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
