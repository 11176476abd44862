#!/usr/bin/env python3
"""What the device minibatch unpack (WarehouseVecEnv.unpack_obs_device, rw_unpack_obs_gather) costs against the path users had before it,
`envs.unpack_obs(tape[idx]).to(dtype)` in torch ops, on the same tensors, and against two floors.  Run on the GPU box from the repository
root, un-profiled:

    python profiles/tools/unpack_gather_ab.py [--out FILE] [--only NAME] [--note TEXT]

Per configuration: an obs_format="packed" env, a rollout tape (T, B, N, PW) written by the fused rollout kernel, random (t, b) groups
drawn with torch.randint (int64), then per element type
    device   unpack_obs_device(tape.reshape(T*B, N, PW), index, dtype, out)
    torch    unpack_obs(tape.reshape(T*B, N, PW)[index]).to(dtype)
each measured two ways (measuring-on-mi355x: events for the device's time, wall clock for what a caller waits):
    kernel   `CALLS` calls enqueued back to back between two events on the env's stream, per call; median of `REPS` such runs
    call     host wall time from the call to the return of envs.sync(), one call at a time; median of `REPS`
and the floors, by events the same way:
    rows     rw_unpack_obs over the same number of CONTIGUOUS rows (float32 only: it has no other type)
    copy     a device-to-device copy of the output's bytes (Tensor.copy_)
The two results are compared bit for bit once per element type before anything is timed."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import rware_amd  # noqa: E402

CALLS, REPS = 20, 7
# name -> (env id, constructor extras, envs, tape steps, groups per minibatch)
CONFIGS = {
    "small-4ag": ("rware-small-4ag-v1", {}, 16384, 64, (16384, 262144)),
    "large-16ag sr2": ("rware-large-16ag-v1", dict(sensor_range=2), 16384, 8, (16384,)),
}
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


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


def by_wall(fn, sync, reps=REPS):
    """us from the call to the return of `sync`, one call at a time, median of `reps`"""
    fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def run(name, emit):
    env_id, extra, B, T, sizes = CONFIGS[name]
    kw = dict(rware_amd.env_kwargs(env_id), **extra)
    env = rware_amd.WarehouseVecEnv(B, output="torch", obs_format="packed", **kw)
    eng = env.engines[0]
    N, L = env.n_agents, eng.L
    env.reset(seed=1)
    actions = torch.randint(0, 5, (T, B, N), dtype=torch.int32, device="cuda")
    tape = env.rollout(actions)[0]
    PW = tape.shape[-1]
    flat = tape.reshape(T * B, N, PW)
    sync = lambda: (env.sync(), torch.cuda.synchronize())
    for n in sizes:
        idx = torch.randint(0, T * B, (n,), device="cuda")
        rows = n * N
        for dname, dt in DTYPES.items():
            out = torch.empty((n, N, L), dtype=dt, device="cuda")
            device = lambda: env.unpack_obs_device(flat, index=idx, dtype=dt, out=out)
            ops = lambda: env.unpack_obs(flat[idx]).to(dt)
            device()
            want = ops()
            sync()
            assert torch.equal(out.view(torch.int32 if dt == torch.float32 else torch.int16),
                               want.view(torch.int32 if dt == torch.float32 else torch.int16)), (name, n, dname)
            del want
            dk, dlo, dhi = by_events(device)
            dc = by_wall(device, sync)
            tk, tlo, thi = by_events(ops, calls=5)
            tc = by_wall(ops, sync)
            nbytes = out.numel() * out.element_size()
            other = torch.empty_like(out)
            ck, _, _ = by_events(lambda: other.copy_(out))
            line = (f"{name}, tape {T} x {B}, {n} groups of {N} rows ({rows * PW * 4 / 1e6:.1f} MB packed -> {nbytes / 1e6:.1f} MB {dname}): "
                    f"device kernel {dk:.1f} us [{dlo:.1f} .. {dhi:.1f}] ({(nbytes + rows * PW * 4) / dk / 1e3:.0f} GB/s read + written), "
                    f"call to sync() {dc:.1f} us | torch ops kernels {tk:.1f} us [{tlo:.1f} .. {thi:.1f}], call to sync() {tc:.1f} us | "
                    f"torch / device {tk / dk:.1f} (kernels), {tc / dc:.1f} (calls) | copy of the output bytes {ck:.1f} us, device / copy {dk / ck:.2f}")
            if dt == torch.float32:
                rk, _, _ = by_events(lambda: eng.unpack_obs_device(flat.data_ptr(), out.data_ptr(), rows))
                line += f" | rw_unpack_obs of {rows} contiguous rows {rk:.1f} us, device / rows {dk / rk:.2f}"
            del other, out
            emit(line)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only")
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# unpack_gather_ab: us, median of {REPS} [min .. max]; un-profiled; {torch.cuda.get_device_name(0)}" + (f"; {args.note}" if args.note else ""))
    for name in CONFIGS:
        if not args.only or args.only in name:
            run(name, emit)


if __name__ == "__main__":
    main()
