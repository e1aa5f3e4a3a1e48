#!/usr/bin/env python
"""Cost of the actuated-joint quantities block (`jm_block_actuation`, `k_actuation`) on ANYmal (12 motors) and Atlas (30 motors).
    python tools/bench_actuation.py [--envs 65536] [--calls 50] [--reps 5] [--steps 20] [--skip-env]
* kernel, `--calls` back-to-back push launches between two device events, `--reps` repetitions in one process (median, min, max
  in microseconds per launch), with windows of `max_stack` 2 and 21, next to the algorithmic bytes per lane: read
  `3 M + M + max_stack` scalars, written `5 M + 3` scalars and 2 integers;
* environment: ms per step of the ANYmal `PDControlledWalkerVecEnv` (constraint contacts) with and without the block, `--reps`
  repetitions of `--steps` steps.  The "without" line runs no code of the block: it is the figure to hold against the same
  environment of an earlier revision.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jiminy_amd import blocks, load_builtin  # noqa: E402
from jiminy_amd.engine import BatchedEngine  # noqa: E402
from jiminy_amd.envs import make_anymal_env  # noqa: E402

STEP_DT = 0.01


def timed(fn, n: int) -> float:
    """Average microseconds per call of `fn` over n calls (device events around the whole loop)."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def summary(samples):
    return {"median": round(statistics.median(samples), 2), "min": round(min(samples), 2), "max": round(max(samples), 2)}


def kernels(model, B: int, dev, calls: int, reps: int) -> dict:
    eng = BatchedEngine(model, B, dtype=torch.float64, device=dev)
    eng.set_options({"stepper": {"odeSolver": "euler_explicit", "dtMax": 1e-3, "controllerUpdatePeriod": 1e-3,
                                 "sensorsUpdatePeriod": 1e-3}})
    q0 = torch.as_tensor(model.neutral(), dtype=torch.float64, device=dev)[:, None].expand(-1, B).contiguous()
    g = torch.Generator(device="cpu").manual_seed(0)
    eng.set_command(torch.randn(model.nmotors, B, generator=g, dtype=torch.float64).to(dev))
    eng.start(q0, torch.zeros((model.nv, B), dtype=torch.float64, device=dev))
    for _ in range(5):
        eng.step(1e-3)
    # horizons of 0.5 and 19.5 steps: windows of 2 and 21 slots
    blocks_ = {s: blocks.ActuatedJointQuantities(eng, generator_mode="CHARGE", power_horizon=h * STEP_DT, power_cutoff=100.0,
                                                 position_margin=0.1, velocity_max=1.0, step_dt=STEP_DT) for s, h in ((2, 0.5), (21, 19.5))}
    M, out = model.nmotors, {"n_motors": model.nmotors}
    samples = {s: [] for s in blocks_}
    for s, blk in blocks_.items():
        assert blk.plan.max_stack == s
        blk.reset()
    for _ in range(reps):       # (interleaved: a drift of the clocks touches every line alike)
        for s, blk in blocks_.items():
            samples[s].append(timed(blk.refresh, calls))
    for s in blocks_:
        read, written = 8 * (3 * M + M + s) + 4, 8 * (5 * M + 3) + 8
        us = summary(samples[s])
        out[f"max_stack_{s}"] = {"k_actuation_us": us, "bytes_read_per_lane": read, "bytes_written_per_lane": written,
                                 "TB_per_s": round((read + written) * B / us["median"] * 1e-6, 2)}
    eng.stop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-env", action="store_true")
    args = ap.parse_args()
    dev, B = torch.device("cuda", 0), args.envs
    out = {"metric": "actuated-joint quantities", "envs": B, "calls": args.calls, "reps": args.reps}
    out["anymal"] = kernels(load_builtin("anymal"), B, dev, args.calls, args.reps)
    out["atlas"] = kernels(load_builtin("atlas"), B, dev, args.calls, args.reps)
    if not args.skip_env:
        g = torch.Generator(device="cpu").manual_seed(0)
        action = (0.3 * torch.randn(B, 12, generator=g, dtype=torch.float64)).to(dev)
        common = dict(device=dev, auto_reset=False, contact_model="constraint")
        cfg = dict(power_horizon=0.2, power_cutoff=100.0, position_margin=0.1, velocity_max=1.0)
        envs = {"without": make_anymal_env(B, **common), "with": make_anymal_env(B, actuated_joints=cfg, **common)}
        samples = {k: [] for k in envs}
        for env in envs.values():
            env.reset(seed=0)
            for _ in range(3):
                env.step(action)
        for _ in range(args.reps):
            for key, env in envs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    env.step(action)
                torch.cuda.synchronize()
                samples[key].append(1e3 * (time.perf_counter() - t0) / args.steps)
        for key, v in samples.items():
            out[f"anymal_env_step_{key}_block_ms"] = summary(v)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
