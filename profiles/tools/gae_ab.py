#!/usr/bin/env python3
"""What advantages and returns from a rollout's tapes cost in one kernel (WarehouseVecEnv.gae_device, rw_gae) against the path users had
before it, the backward loop over T in torch ops, on the same tensors, and against the rollout that produced the tape and a copy of the
bytes.  Run on the GPU box from the repository root, un-profiled:

    python profiles/tools/gae_ab.py [--out FILE] [--only NAME] [--note TEXT]

Per configuration: an env with time_limit_truncates (so that both kinds of end occur), a rollout tape of T steps written by the fused
rollout kernel under random actions, random values, then
    device   gae_device(rewards, values, terminated, truncated, prev_ended=..., out=...)
    torch    the same recurrence as a loop of T iterations of elementwise tensor ops (torch_gae below: what a PPO implementation writes)
each measured two ways (measuring-on-mi355x: events for the device's time, wall clock for what a caller waits):
    kernel   `CALLS` calls enqueued back to back between two events on the env's stream, per call; median of `REPS` such runs
    call     host wall time from the call to the return of envs.sync(), one call at a time; median of `REPS`
and, by events the same way, the rollout() that wrote the tape and a device-to-device copy of the two float outputs' bytes.
The device result is compared with rware_amd.gae bit for bit, and the torch loop with it to 1e-4, before anything is timed."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rware_amd  # noqa: E402

CALLS, REPS = 20, 7
# name -> (env id, envs, tape steps, max_steps, value heads: "agents" or 1)
CONFIGS = {
    "small-4ag per-agent": ("rware-small-4ag-v1", 16384, 64, 25, "agents"),
    "small-4ag team": ("rware-small-4ag-v1", 16384, 64, 25, 1),
    "large-16ag per-agent": ("rware-large-16ag-v1", 4096, 64, 25, "agents"),
    "large-16ag team": ("rware-large-16ag-v1", 4096, 64, 25, 1),
    "tiny-2ag 1024 per-agent": ("rware-tiny-2ag-v1", 1024, 64, 25, "agents"),
}


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


def torch_gae(rew, val, term, trunc, prev, gamma, lam, team):
    """GAE under NEXT_STEP autoreset in tensor ops: -> (advantages, returns, valid).  values (T+1, B, K); flags bool."""
    T = rew.shape[0]
    r = rew.sum(dim=2, keepdim=True) if team else rew
    ended = term | trunc
    reset = torch.cat([prev[None], ended[:-1]])
    adv = torch.empty_like(val[:T])
    carry = torch.zeros_like(val[0])
    for t in range(T - 1, -1, -1):
        delta = r[t] + gamma * val[t + 1] * (~term[t])[:, None] - val[t]
        carry = delta + gamma * lam * (~ended[t])[:, None] * carry
        carry = carry * (~reset[t])[:, None]
        adv[t] = carry
    return adv, adv + val[:T], ~reset


def run(name, emit):
    env_id, B, T, max_steps, heads = CONFIGS[name]
    kw = dict(rware_amd.env_kwargs(env_id), max_steps=max_steps, time_limit_truncates=True)
    env = rware_amd.WarehouseVecEnv(B, output="torch", **kw)
    N = env.n_agents
    K = N if heads == "agents" else 1
    env.reset(seed=1)
    actions = torch.randint(0, 5, (T, B, N), dtype=torch.int32, device="cuda")
    _, rew, term, trunc = env.rollout(actions, want_obs=False)
    prev = torch.zeros(B, dtype=torch.bool, device="cuda")
    val = torch.randn((T + 1, B, K), device="cuda")
    outs = (torch.empty((T, B, K), device="cuda"), torch.empty((T, B, K), device="cuda"), torch.empty((T, B), dtype=torch.bool, device="cuda"))
    sync = lambda: (env.sync(), torch.cuda.synchronize())
    device = lambda: env.gae_device(rew, val, term, trunc, prev_ended=prev, out=outs)
    ops = lambda: torch_gae(rew, val, term, trunc, prev, 0.99, 0.95, K == 1 and N > 1)
    device()
    want_t = ops()
    sync()
    want = rware_amd.gae(rew.cpu().numpy(), val.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), prev_ended=prev.cpu().numpy())
    for got, w, wt in zip(outs, want, want_t):
        g = got.cpu().numpy()
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
        assert np.allclose(g.astype(np.float32), wt.cpu().numpy().astype(np.float32), atol=1e-4), name
    ends = int((term | trunc).sum())
    del want_t
    dk, dlo, dhi = by_events(device)
    dc = by_wall(device, sync)
    tk, tlo, thi = by_events(ops, calls=3, reps=5)
    tc = by_wall(ops, sync, reps=5)
    rk, _, _ = by_events(lambda: env.rollout(actions, want_obs=False), calls=5)
    other = torch.empty_like(outs[0])
    ck, _, _ = by_events(lambda: (other.copy_(outs[0]), other.copy_(outs[1])))
    moved = (rew.numel() + val.numel() + 2 * outs[0].numel()) * 4 + 5 * T * B
    emit(f"{name}: tape {T} x {B} x {N}, {K} heads ({moved / 1e6:.1f} MB read + written, {ends} ends): device kernel {dk:.1f} us [{dlo:.1f} .. {dhi:.1f}] "
         f"({moved / dk / 1e3:.0f} GB/s), call to sync() {dc:.1f} us | torch loop kernels {tk:.1f} us [{tlo:.1f} .. {thi:.1f}], call to sync() {tc:.1f} us | "
         f"torch / device {tk / dk:.1f} (kernels), {tc / dc:.1f} (calls) | the rollout of the tape (no observations) {rk:.1f} us, device / rollout {dk / rk:.2f}, "
         f"torch / rollout {tk / rk:.1f} | copy of the two float outputs {ck:.1f} us, device / copy {dk / ck:.2f}")
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

    emit(f"# gae_ab: us, median of {REPS} [min .. max]; un-profiled; {torch.cuda.get_device_name(0)}" + (f"; {args.note}" if args.note else ""))
    for name in CONFIGS:
        if not args.only or args.only in name:
            run(name, emit)


if __name__ == "__main__":
    main()
