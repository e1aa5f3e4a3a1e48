#!/usr/bin/env python
"""Cost of the DeformationEstimator block on the authored flexible arm (tests/data/flex_arm.urdf).
    python tools/bench_deformation.py [--envs 65536] [--calls 50] [--steps 20]
* kernels: `jm_block_deformation_estimator` (4 flexibility points, 4 IMUs, 2 encoders) and `jm_block_mahony_filter` of the
  same robot, `--calls` launches each, timed with device events;
* environment: ms per step of `PDControlledWalkerVecEnv` on the free-flyer arm with and without the block.
Prints one JSON line.  Kernel durations proper come from a profiler run of this script:
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/bench_deformation.py
    python tools/rocpd_stats.py <dir> 14"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jiminy_amd import blocks  # noqa: E402
from jiminy_amd.engine import BatchedEngine  # noqa: E402
from jiminy_amd.envs import PDControlledWalkerVecEnv  # noqa: E402
from tests import robots_deformation as rd  # noqa: E402


def timed(fn, n: int) -> float:
    """Average milliseconds per call of `fn` over n calls (device events around the whole loop)."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    dev, B = torch.device("cuda", 0), args.envs
    out = {"metric": "DeformationEstimator block, flex_arm", "envs": B}

    model = rd.flex_arm(False)
    eng = BatchedEngine(model, B, dtype=torch.float64, device=dev)
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": 1e-3, "controllerUpdatePeriod": 1e-3,
                                 "sensorsUpdatePeriod": 1e-3}})
    q0 = torch.as_tensor(model.neutral(), dtype=torch.float64, device=dev)[:, None].expand(-1, B).contiguous()
    eng.start(q0, torch.zeros((model.nv, B), dtype=torch.float64, device=dev))
    for _ in range(20):
        eng.step(1e-3)
    n_imu = len(model.sensors["ImuSensor"])
    quat = torch.zeros((4, n_imu, B), dtype=torch.float64, device=dev)
    quat[3] = 1.0
    bias, omega, cf = (torch.zeros((3, n_imu, B), dtype=torch.float64, device=dev) for _ in range(3))
    hb = blocks.HipBlocks(eng, [1, 0], torch.zeros(3, 2), torch.zeros(3, 2), torch.ones(2), torch.ones(2), torch.ones(2))
    for ignore_twist in (True, False):
        est = blocks.DeformationEstimator(eng, rd.imu_frames(False), list(rd.FLEX_FRAMES), ignore_twist=ignore_twist)
        key = "swing" if ignore_twist else "twist"
        out[f"deformation_estimator_{key}_ms"] = timed(lambda: est.refresh(quat), args.calls)
    out["mahony_filter_ms"] = timed(lambda: hb.mahony_filter(quat, omega, cf, bias, 1.0, 0.1, 1e-3), args.calls)
    del eng, hb, est

    ff = rd.flex_arm(True)
    cfg = dict(imu_frame_names=rd.imu_frames(True), flex_frame_names=list(rd.FLEX_FRAMES))
    g = torch.Generator(device="cpu").manual_seed(0)
    action = ((torch.rand(B, 2, generator=g, dtype=torch.float64) - 0.5) * 0.5).to(dev)
    for key, kw in (("without", {}), ("with", {"deformation_estimator": cfg})):
        env = PDControlledWalkerVecEnv(ff, B, step_dt=0.01, control_dt=0.005, kp=[20.0, 20.0], kd=[0.05, 0.05], device=dev,
                                       engine_options={"stepper": {"odeSolver": "runge_kutta_4", "dtMax": 1e-3}},
                                       auto_reset=False, **kw)
        env.reset(seed=0)
        for _ in range(3):
            env.step(action)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            env.step(action)
        torch.cuda.synchronize()
        out[f"env_step_{key}_block_ms"] = 1e3 * (time.perf_counter() - t0) / args.steps
        del env
    print(json.dumps(out))


if __name__ == "__main__":
    main()
