#!/usr/bin/env python
"""Cost of the tracking windows block (`jm_block_tracking`, `k_tracking`) at the sizes of ANYmal (3 relative feet, 12 motors) and
Atlas (1 relative foot, 30 motors).
    python tools/bench_tracking.py [--envs 65536] [--calls 50] [--reps 5] [--steps 20] [--skip-env]
* kernel, `--calls` back-to-back push launches between two device events, `--reps` repetitions in one process (median, min, max
  in microseconds per launch), the three families on windows of `max_stack` 2 and 26 (one second at the 0.04 s environment
  step), next to the algorithmic bytes per lane: read 6 + 14 R + 2 M scalars of the sources, 4 of the oldest odometry slot, 2 of
  the previous yaws and 2 (S - 2) + 2 (S - 1) + (S - 1) of the rings, a counter; written 4 + 2 + 2 + 2 + 1 state scalars, 6 + 6
  outputs, a counter.  The source tensors are random: the kernel's work does not depend on their values;
* environment: ms per step of the ANYmal `PDControlledWalkerVecEnv` (constraint contacts) with and without the block (and the
  three blocks it reads), `--reps` repetitions of `--steps` steps.  The "without" line runs no code of the block: it is the
  figure to hold against the same environment of an earlier revision.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jiminy_amd import blocks, load_builtin  # noqa: E402
from jiminy_amd.engine import BatchedEngine  # noqa: E402
from jiminy_amd.envs import make_anymal_env  # noqa: E402

STEP_DT = 0.04


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


def kernels(model, n_feet: int, B: int, dev, calls: int, reps: int) -> dict:
    eng = BatchedEngine(model, B, dtype=torch.float64, device=dev)
    eng.set_options({"stepper": {"odeSolver": "euler_explicit", "dtMax": 1e-3, "controllerUpdatePeriod": 1e-3,
                                 "sensorsUpdatePeriod": 1e-3}})
    q0 = torch.as_tensor(model.neutral(), dtype=torch.float64, device=dev)[:, None].expand(-1, B).contiguous()
    eng.start(q0, torch.zeros((model.nv, B), dtype=torch.float64, device=dev))
    g = torch.Generator(device="cpu").manual_seed(0)
    R, M = n_feet - 1, model.nmotors
    rand = lambda *shape: torch.randn(*shape, B, generator=g, dtype=torch.float64).to(dev)      # noqa: E731
    # stand-ins of the three source blocks: the tensors the kernel reads, of the right shapes
    loco = SimpleNamespace(_eng=eng, odom_pose=rand(3))
    feet = SimpleNamespace(_eng=eng, relative_pose=rand(7, R), reference_relative_pose=rand(7, R), plan=SimpleNamespace(n_feet=n_feet),
                           foot_frame_names=[])
    act = SimpleNamespace(_eng=eng, position=rand(M), motor_side=False, plan=SimpleNamespace(n_motors=M, motor_names=[]))
    # horizons of 0.5 and 24.5 steps: windows of 2 and 26 slots (a horizon below a step is refused: 1 step gives 2 slots)
    blocks_ = {s: blocks.TrackingWindows(eng, locomotion=loco, foot_poses=feet, actuation=act, odometry_horizon=h * STEP_DT,
                                         foot_horizon=h * STEP_DT, motor_horizon=h * STEP_DT, odometry_cutoff=0.5, step_dt=STEP_DT)
               for s, h in ((2, 1.0), (26, 24.5))}
    out = {"n_rel": R, "n_motors": M}
    samples = {s: [] for s in blocks_}
    for s, blk in blocks_.items():
        p = blk.plan
        assert (p.max_stack_odom, p.max_stack_foot, p.max_stack_motor) == (s, s, s)
        blk.reference_odom_pose.copy_(rand(3))
        blk.reference_position.copy_(rand(M))
        blk.reset()
        for _ in range(s):      # (the windows are full before the clock starts)
            blk.refresh()
    for _ in range(reps):       # (interleaved: a drift of the clocks touches every line alike)
        for s, blk in blocks_.items():
            samples[s].append(timed(blk.refresh, calls))
    for s in blocks_:
        read = 8 * (6 + 14 * R + 2 * M + 4 + 2 + 2 * (s - 2) + 2 * (s - 1) + (s - 1)) + 4
        written = 8 * (4 + 2 + 2 + 2 + 1 + 6 + 6) + 4
        us = summary(samples[s])
        out[f"max_stack_{s}"] = {"k_tracking_us": us, "bytes_read_per_lane": read, "bytes_written_per_lane": written,
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
    out = {"metric": "tracking windows", "envs": B, "calls": args.calls, "reps": args.reps}
    out["anymal"] = kernels(load_builtin("anymal"), 4, B, dev, args.calls, args.reps)
    out["atlas"] = kernels(load_builtin("atlas"), 2, B, dev, args.calls, args.reps)
    if not args.skip_env:
        g = torch.Generator(device="cpu").manual_seed(0)
        action = (0.3 * torch.randn(B, 12, generator=g, dtype=torch.float64)).to(dev)
        common = dict(device=dev, auto_reset=False, contact_model="constraint")
        cfg = dict(locomotion_quantities=dict(forces=False, momentum=False), foot_poses={}, actuated_joints={},
                   trajectory_tracking=dict(odometry_horizon=1.0, foot_horizon=1.0, motor_horizon=1.0, odometry_cutoff=0.5))
        envs = {"without": make_anymal_env(B, **common), "with": make_anymal_env(B, **cfg, **common)}
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
