#!/usr/bin/env python
"""Cost of the foot pose quantities block (`jm_block_foot_poses`, `k_foot_poses`) on ANYmal (4 feet: the eigen branch) and
Atlas (2 feet: the midpoint branch).
    python tools/bench_footposes.py [--envs 65536] [--calls 50] [--reps 5] [--steps 20] [--skip-env]
* kernel, `--calls` back-to-back launches between two device events, `--reps` repetitions in one process (median, min, max in
  microseconds per launch): the block with every output, a reference and both reward rows, next to the launch of the frame
  kinematics block it reads (the yardstick), and the bytes a lane moves (two passes over the rows of the feet, the reference,
  every output);
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
from jiminy_amd.locomotion import sanitize_foot_frame_names  # noqa: E402


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
                                 "sensorsUpdatePeriod": 1e-3}, "contacts": {"model": "constraint"}})
    q0 = torch.as_tensor(model.neutral(), dtype=torch.float64, device=dev)[:, None].expand(-1, B).contiguous()
    eng.start(q0, torch.zeros((model.nv, B), dtype=torch.float64, device=dev))
    for _ in range(5):
        eng.step(1e-3)
    fk = blocks.FrameKinematics(eng, sanitize_foot_frame_names(model), compute_velocity=False)
    fp = blocks.FootPoseQuantities(eng, fk, position_cutoff=0.1, orientation_cutoff=0.5)
    fk.reset()
    fp.reset()
    lines = {"k_foot_poses": fp.refresh, "k_frame_kinematics": fk.refresh}
    samples = {k: [] for k in lines}
    for _ in range(reps):       # (interleaved: a drift of the clocks touches every line alike)
        for k, fn in lines.items():
            samples[k].append(timed(fn, calls))
    eng.stop()
    F = fp.plan.n_feet
    read_rows, written_rows = 7 * F + 7 * (F - 1) + 7 * (F - 1), 7 + 3 + 7 * (F - 1) + 6 * (F - 1) + 2
    return {"n_feet": F, "bytes_per_lane": 8 * (read_rows + written_rows), **{k + "_us": summary(v) for k, v in samples.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-env", action="store_true")
    args = ap.parse_args()
    dev, B = torch.device("cuda", 0), args.envs
    out = {"metric": "foot pose quantities", "envs": B, "calls": args.calls, "reps": args.reps}
    out["anymal"] = kernels(load_builtin("anymal"), B, dev, args.calls, args.reps)
    out["atlas"] = kernels(load_builtin("atlas"), B, dev, args.calls, args.reps)
    if not args.skip_env:
        g = torch.Generator(device="cpu").manual_seed(0)
        action = (0.3 * torch.randn(B, 12, generator=g, dtype=torch.float64)).to(dev)
        common = dict(device=dev, auto_reset=False, contact_model="constraint")
        envs = {"without": make_anymal_env(B, **common),
                "with": make_anymal_env(B, foot_poses=dict(position_cutoff=0.1, orientation_cutoff=0.5), **common)}
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
