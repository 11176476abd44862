#!/usr/bin/env python3
"""What the device form of get_global_image costs and saves (rw_global_image), and that the per-step time did not move.  Same box, un-profiled.

    global_image_ab.py [--parent-lib PATH/librware_hip.so] [--out FILE] [--reps 5] [--image-reps 30] [--steps 2000] [--warmup 200]

Per configuration (small-4ag x 16384, x 262144, large-16ag x 16384; layers SHELVES, REQUESTS, AGENTS, GOALS, ACCESSIBLE) one process with
one output="torch" env, 20 random steps into its episodes:
(a) host    env.get_global_image(layers, recompute=True): get_state() — the int32 grid and the agent arrays to the host — then numpy;
            host wall time, call to result.
(b) device  env.global_image_device(layers, dtype=...) float32 and uint8: host wall time from the call to the return of env.sync() behind
            it, and to the return of the call itself (the enqueue).  Forms (a) and (b) are warmed, then alternate `--image-reps` times;
            median and (max - min) / median.  The first device call behind the host form — the first launch after tens of milliseconds
            in which the process enqueued nothing — is timed apart (its enqueue alone): what a loop that calls every step does not pay.
(c) kernel  100 calls captured into one HIP graph on a stream of the env's own and replayed five times between two events: us per launch
            (median of the five), against rw_debug_store_floor — a launch that only stores — of a second engine of the same configuration
            whose observation buffer has the byte count of the float32 image (its batch is chosen for that; the figure is scaled by
            the remaining ratio of the two byte counts, printed beside it).
(d) per-step time, default small-4ag x 16384 engine, this tree's library against the PARENT commit's (`--parent-lib`; it travels as a .so):
    one process per leg driving the C-ABI directly, a device tape of 64 random action rows, `--warmup` untimed steps, then `--steps` steps
    timed with the engine's events riding on the first / last dispatch.  Legs a (parent), b (this tree), a (parent again) alternate
    `--reps` times; reported: b / a on the medians beside the parent-against-parent spread, (max - min) / median over all parent runs."""
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
LAYERS = [0, 1, 2, 5, 6]
CONFIGS = [("rware-small-4ag-v1", 16384), ("rware-small-4ag-v1", 262144), ("rware-large-16ag-v1", 16384)]


def image_leg(args):
    import numpy as np
    import torch

    import rware_amd

    B = args.batch
    kw = rware_amd.env_kwargs(args.env_id)
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
    for _ in range(args.image_reps if B <= 65536 else max(5, args.image_reps // 5)):   # (the host form takes seconds at 262144 envs)
        out["host"].append(host()[0])
        out["f32_first"].append(device("float32")[1])   # the first launch behind tens of ms of host work: its enqueue alone, kept apart
        for key, dtype in (("f32", "float32"), ("u8", "uint8")):
            total, enq, _ = device(dtype)
            out[key].append(total)
            out[key + "_enq"].append(enq)
    res = {k: [1e6 * x for x in v] for k, v in out.items()}
    # (c) the kernel alone: captured launches replayed between two events on a stream of the env's own
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
    # the store-only launch: an engine whose float32 observation buffer is as large as the float32 image
    obs_bytes_per_env = env.n_agents * env.obs_length * 4
    Bf = max(64, int(round(res["f32_bytes"] / obs_bytes_per_env / 64.0)) * 64)
    floor_env = rware_amd.WarehouseVecEnv(Bf, **kw)
    floor_env.reset(seed=1)
    floor_env.sync()
    floor_us = 1e3 * floor_env.engines[0].debug_store_floor(200)
    res["floor_bytes"] = Bf * obs_bytes_per_env
    res["floor_us_same_bytes"] = floor_us * res["f32_bytes"] / res["floor_bytes"]
    floor_env.close()
    env.close()
    print(json.dumps(res))


def step_leg(args):
    import numpy as np

    import rware_amd
    from rware_amd import _capi

    B = 16384
    kw = rware_amd.env_kwargs("rware-small-4ag-v1")
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
    ap.add_argument("--env-id")
    ap.add_argument("--batch", type=int)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--image-reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    if args.leg == "image":
        return image_leg(args)
    if args.leg == "step":
        return step_leg(args)
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    cell = lambda v: f"{med(v):.1f} ({100 * spread(v):.0f} %)"
    lines = [f"# (a) (b) the global image, layers {LAYERS}: host wall time in us; median of {args.image_reps} alternations ({max(5, args.image_reps // 5)} beyond 65536 envs) ((max - min) / median), "
             "after 3 warm-up rounds of every form; un-profiled",
             "# config | (a) host: get_global_image(recompute=True) | (b) device float32, call to sync() | its call alone | device uint8, call to "
             "sync() | its call alone | host / device float32 | host / device uint8 | the first call behind the host form, call alone"]
    kernel = ["", "# (c) the kernel alone: us per launch, 100 captured launches per replay, median of 5 replays; store-only = rw_debug_store_floor of an "
              "engine whose observation buffer has the float32 image's byte count (scaled by the remaining ratio)",
              "# config | image MB float32 | kernel float32 us (GB/s) | kernel uint8 us (GB/s) | store-only us, same bytes as float32 (GB/s) | kernel float32 / store-only"]
    for env_id, B in CONFIGS:
        r = child(["--leg", "image", "--env-id", env_id, "--batch", str(B), "--image-reps", str(args.image_reps)])
        name = f"{env_id.replace('rware-', '').replace('-v1', '')} x {B}"
        lines.append(f"{name} | {cell(r['host'])} | {cell(r['f32'])} | {cell(r['f32_enq'])} | {cell(r['u8'])} | {cell(r['u8_enq'])} | "
                     f"{med(r['host']) / med(r['f32']):.1f} | {med(r['host']) / med(r['u8']):.1f} | {cell(r['f32_first'])}")
        gbs = lambda b, us: b / us / 1e3
        kernel.append(f"{name} | {r['f32_bytes'] / 1e6:.1f} | {r['f32_kernel_us']:.1f} ({gbs(r['f32_bytes'], r['f32_kernel_us']):.0f}) | "
                      f"{r['u8_kernel_us']:.1f} ({gbs(r['u8_bytes'], r['u8_kernel_us']):.0f}) | "
                      f"{r['floor_us_same_bytes']:.1f} ({gbs(r['f32_bytes'], r['floor_us_same_bytes']):.0f}; measured on {r['floor_bytes'] / 1e6:.1f} MB) | "
                      f"{r['f32_kernel_us'] / r['floor_us_same_bytes']:.2f}")
        print(lines[-1], flush=True)
        print(kernel[-1], flush=True)
    lines += kernel
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
        lines += ["", f"# (d) us per step, default rware-small-4ag-v1 x 16384 engine, {args.steps} timed steps after {args.warmup}; a = parent commit's library "
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
