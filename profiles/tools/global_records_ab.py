#!/usr/bin/env python3
"""What the critic's global state costs as byte records (rw_global_records, rw_global_image_gather) against the images a learner had to
keep before them, and against floors.  Run on the GPU box from the repository root, un-profiled:

    python profiles/tools/global_records_ab.py [--out FILE] [--only NAME] [--parent-lib PATH/librware_hip.so] [--note TEXT]

Per configuration, an output="torch" env 20 random steps into its episodes; kernels by events (`CALLS` calls enqueued back to back between
two events, per call; median of `REPS` such runs, [min .. max]):
    (a) per step   rw_global_records against rw_global_image uint8 with the five default layers on the same engine, and against a
                   device-to-device copy of the B * RB record bytes
    (b) minibatch  a T-step tape of records (global_records_device(out=tape[t]) behind every step) and the uint8 image tape of the same
                   steps; n random records drawn with torch.randint (int64), per element type
                       device   global_image_from_records(tape, index, PLAIN, dtype, out)
                       torch    tape_u8[index].to(dtype)
                   and a copy of the output's bytes as the floor; the two results are compared bit for bit before anything is timed
    (c) bytes      of the tape per step: records, uint8 images, float32 images
With --parent-lib:
    (d') rw_global_image itself, float32 and uint8, parent / this / parent in child processes that alternate five times (its kernel is
         now build + expand out of rware_global_state.h): this / parent on the medians against what single parent runs give against each
         other.  The per-step time of the step kernels is `ab.py baseline`'s business."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rware_amd  # noqa: E402
from rware_amd import _capi  # noqa: E402

CALLS, REPS = 20, 7
PLAIN = [0, 1, 2, 5, 6]
# name -> (env id, envs, tape steps, records per minibatch)
CONFIGS = {
    "small-4ag x 16384": ("rware-small-4ag-v1", 16384, 64, (16384, 262144)),
    "small-4ag x 262144": ("rware-small-4ag-v1", 262144, 0, ()),
    "large-16ag x 16384": ("rware-large-16ag-v1", 16384, 64, (16384, 262144)),
}
DTYPES = {"float32": torch.float32, "uint8": torch.uint8, "float16": torch.float16, "bfloat16": torch.bfloat16}
VIEWS = {torch.float32: torch.int32, torch.uint8: torch.uint8, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def by_events(fn, calls=CALLS, reps=REPS):
    """us per call: `calls` calls between two events on the current stream, median of `reps` (after one untimed run)"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return statistics.median(out), min(out), max(out)


def played(env_id, B, library=None):
    env = rware_amd.WarehouseVecEnv(B, output="torch", library=library, **rware_amd.env_kwargs(env_id))
    env.reset(seed=1)
    step(env, 20, np.random.default_rng(0))
    env.sync()
    return env


def step(env, n, rng, each=None):
    for t in range(n):
        env.step(torch.from_numpy(rng.choice(5, size=(env.num_envs, env.n_agents), p=[.1, .5, .15, .15, .1]).astype(np.int32)).cuda())
        if each:
            each(t)


def run(name, emit):
    env_id, B, T, sizes = CONFIGS[name]
    env = played(env_id, B)
    eng = env.engines[0]
    H, W = env.grid_size
    rb = env.global_record_bytes
    sync = lambda: (env.sync(), torch.cuda.synchronize())
    # (a)
    rec = env.global_records_device()
    img8 = env.global_image_device(PLAIN, dtype="uint8")
    sync()
    other = torch.empty_like(rec)
    rk, rlo, rhi = by_events(lambda: eng.global_records(rec.data_ptr()))
    ik, ilo, ihi = by_events(lambda: eng.global_image(PLAIN, img8.data_ptr(), None, np.uint8))
    ck, _, _ = by_events(lambda: other.copy_(rec))
    emit(f"(a) {name}, {H} x {W}, RB {rb}: rw_global_records {rk:.1f} us [{rlo:.1f} .. {rhi:.1f}] for {rec.numel() / 1e6:.1f} MB | rw_global_image uint8, "
         f"five layers {ik:.1f} us [{ilo:.1f} .. {ihi:.1f}] for {img8.numel() / 1e6:.1f} MB | records / image {rk / ik:.2f} | copy of the record bytes "
         f"{ck:.1f} us, records / copy {rk / ck:.2f}")
    # (c)
    emit(f"(c) {name}: tape bytes per step: records {B * rb / 1e6:.2f} MB, uint8 images (five layers) {B * 5 * H * W / 1e6:.2f} MB, float32 images "
         f"{B * 20 * H * W / 1e6:.2f} MB; per cell {rb / (H * W):.2f} / 5 / 20 bytes")
    del other
    # (b)
    if T:
        tape = torch.empty((T, B, rb), dtype=torch.uint8, device="cuda")
        tape_u8 = torch.empty((T, B, 5, H, W), dtype=torch.uint8, device="cuda")

        def keep(t):
            env.global_records_device(out=tape[t])
            env.global_image_device(PLAIN, dtype="uint8", out=tape_u8[t])

        step(env, T, np.random.default_rng(1), keep)
        sync()
        flat_u8 = tape_u8.reshape(T * B, 5, H, W)
        for n in sizes:
            idx = torch.randint(0, T * B, (n,), device="cuda")
            for dname, dt in DTYPES.items():
                out = torch.empty((n, 5, H, W), dtype=dt, device="cuda")
                device = lambda: env.global_image_from_records(tape, idx, PLAIN, dtype=dt, out=out)
                ops = lambda: flat_u8[idx].to(dt)
                device()
                want = ops()
                sync()
                assert torch.equal(out.view(VIEWS[dt]), want.view(VIEWS[dt])), (name, n, dname)
                del want
                dk, dlo, dhi = by_events(device)
                tk, tlo, thi = by_events(ops, calls=5)
                nbytes = out.numel() * out.element_size()
                other = torch.empty_like(out)
                ck, _, _ = by_events(lambda: other.copy_(out))
                emit(f"(b) {name}, tape {T} x {B}, {n} records ({n * rb / 1e6:.1f} MB of records -> {nbytes / 1e6:.1f} MB {dname}): device kernel "
                     f"{dk:.1f} us [{dlo:.1f} .. {dhi:.1f}] ({(nbytes + n * rb) / dk / 1e3:.0f} GB/s read + written) | torch ops on the uint8 image tape "
                     f"{tk:.1f} us [{tlo:.1f} .. {thi:.1f}] | torch / device {tk / dk:.1f} | copy of the output bytes {ck:.1f} us, device / copy {dk / ck:.2f}")
                del other, out
    env.close()


def image_child(lib):
    """rw_global_image on `lib`, small-4ag x 16384: one JSON line, us per launch by events"""
    try:
        _capi.load(lib)
    except AttributeError:   # (the parent's library has everything but this header's entry points)
        del _capi.HEADERS["rware_hip_global_state.h"]
    env = played("rware-small-4ag-v1", 16384, library=lib)
    eng = env.engines[0]
    res = {}
    for key, dt in (("float32", np.float32), ("uint8", np.uint8)):
        img = env.global_image_device(PLAIN, dtype=key)
        env.sync()
        res[key] = by_events(lambda: eng.global_image(PLAIN, img.data_ptr(), None, dt), calls=50)[0]
    env.close()
    print(json.dumps(res))


def image_ab(parent, emit, reps=5):
    own = os.path.join(ROOT, "robotic-warehouse_amd", "csrc", "librware_hip.so")
    runs = {"a": [], "b": [], "a2": []}
    for _ in range(reps):
        for leg, lib in (("a", parent), ("b", own), ("a2", parent)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--image-child", lib], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                raise SystemExit(f"leg {leg} failed with exit status {out.returncode}: {out.stderr[-400:]}")
            runs[leg].append(json.loads(out.stdout.strip().splitlines()[-1]))
    for key in ("float32", "uint8"):
        med = {leg: statistics.median(r[key] for r in v) for leg, v in runs.items()}
        parents = [r[key] for r in runs["a"] + runs["a2"]]
        pm = statistics.median(parents)
        lo, hi = min(parents) / pm, max(parents) / pm
        ratio = med["b"] / statistics.median(parents)
        emit(f"(d') rw_global_image {key}, small-4ag x 16384, five layers, {reps} alternations: parent {med['a']:.2f} / this {med['b']:.2f} / parent "
             f"{med['a2']:.2f} us; this / parent {ratio:.4f}; single parent runs against their median {lo:.4f} .. {hi:.4f}: "
             f"{'inside' if lo <= ratio <= hi else 'OUTSIDE'} the spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only")
    ap.add_argument("--note", default="")
    ap.add_argument("--parent-lib")
    ap.add_argument("--image-child")
    args = ap.parse_args()
    if args.image_child:
        return image_child(args.image_child)
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# global_records_ab: us, median of {REPS} [min .. max]; un-profiled; {torch.cuda.get_device_name(0)}" + (f"; {args.note}" if args.note else ""))
    for name in CONFIGS:
        if not args.only or args.only in name:
            run(name, emit)
    if args.parent_lib:
        image_ab(args.parent_lib, emit)


if __name__ == "__main__":
    main()
