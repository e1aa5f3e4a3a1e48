#!/usr/bin/env python
"""Cost of the attitude observers (MahonyFilter with its options, BodyObserver) on ANYmal (1 IMU) and on the authored
flexible arm (tests/data/flex_arm.urdf, 4 IMUs).
    python tools/bench_attitude.py [--envs 65536] [--calls 50] [--reps 5] [--steps 20]
* kernels, `--calls` back-to-back launches each between two device events, `--reps` repetitions (median, min, max in
  microseconds per launch): `jm_block_mahony_filter` (`k_mahony`, the plain function around the same `mahony_lane`: the yardstick),
  `jm_block_mahony_observer` with every option off and with twist removal + Euler angles, `jm_block_body_observer`
  (twist integrated, Euler angles), `jm_block_attitude_init` (exact);
* environment: ms per step of the ANYmal `PDControlledWalkerVecEnv` with and without the two blocks, `--reps` repetitions of
  `--steps` steps.
Prints one JSON line.  Kernel durations proper come from a profiler run of this script:
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/bench_attitude.py --reps 1"""
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
from tests import robots_deformation as rd  # noqa: E402


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
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": 1e-3, "controllerUpdatePeriod": 1e-3,
                                 "sensorsUpdatePeriod": 1e-3}})
    q0 = torch.as_tensor(model.neutral(), dtype=torch.float64, device=dev)[:, None].expand(-1, B).contiguous()
    eng.start(q0, torch.zeros((model.nv, B), dtype=torch.float64, device=dev))
    for _ in range(20):
        eng.step(1e-3)
    M = model.nmotors
    hb = blocks.HipBlocks(eng, list(range(M)), torch.zeros(3, M), torch.zeros(3, M), torch.ones(M), torch.ones(M), torch.ones(M))
    plain = blocks.MahonyFilter(eng)
    full = blocks.MahonyFilter(eng, ignore_twist=True, compute_rpy=True)
    body = blocks.BodyObserver(eng, full, twist_time_constant=0.5)
    for m in (plain, full):
        m.reset()
    body.reset()
    lines = {
        "k_mahony": lambda: hb.mahony_filter(plain.quat, plain.omega, plain._cf, plain.bias, 1.0, 0.1, 1e-3),
        "k_mahony_observer_plain": lambda: plain.refresh(1e-3),
        "k_mahony_observer_swing_rpy": lambda: full.refresh(1e-3),
        "k_body_observer": lambda: body.refresh(1e-3),
        "k_attitude_init": lambda: full.reset(),
    }
    samples = {k: [] for k in lines}
    for _ in range(reps):       # (interleaved: a drift of the clocks touches every line alike)
        for k, fn in lines.items():
            samples[k].append(timed(fn, calls))
    return {"n_imu": plain.plan.n_imu, **{k + "_us": summary(v) for k, v in samples.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    dev, B = torch.device("cuda", 0), args.envs
    out = {"metric": "attitude observers", "envs": B, "calls": args.calls, "reps": args.reps}
    out["anymal"] = kernels(load_builtin("anymal"), B, dev, args.calls, args.reps)
    out["flex_arm"] = kernels(rd.flex_arm(False), B, dev, args.calls, args.reps)

    g = torch.Generator(device="cpu").manual_seed(0)
    action = (0.3 * torch.randn(B, 12, generator=g, dtype=torch.float64)).to(dev)
    cfg = dict(mahony_filter=dict(ignore_twist=True, compute_rpy=True), body_observer=dict(twist_time_constant=0.5))
    envs = {"without": make_anymal_env(B, device=dev, auto_reset=False), "with": make_anymal_env(B, device=dev, auto_reset=False, **cfg)}
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
        out[f"anymal_env_step_{key}_blocks_ms"] = summary(v)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
