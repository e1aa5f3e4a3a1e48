#!/usr/bin/env python
"""Cost of the frame kinematics block on ANYmal: root joint, the four feet and the IMU frame.
    python tools/bench_frames.py [--envs 65536] [--calls 200] [--reps 5]
`--calls` back-to-back launches between two device events, `--reps` repetitions, interleaved over the lines (median, min, max
in microseconds per launch), float64 and float32:
* `k_frame_kinematics` with the pose alone, with pose + Euler angles + velocity, and as the reset (the previous pose too);
* `k_frame_average` with its three outputs.
Next to every line the bytes the algorithm needs -- (rows read + rows written) * sizeof(T) * B, `q` and `v` counted once -- and the
time the HBM would need for them at its peak rate (MI355X: 8 TB/s).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jiminy_amd import blocks, load_builtin  # noqa: E402
from jiminy_amd.engine import BatchedEngine  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def timed(fn, n: int) -> float:
    """Average microseconds per call of `fn` over n calls (device events around the whole loop)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev, B = torch.device("cuda", 0), args.envs
    model = load_builtin("anymal")
    names = ["root_joint"] + list(model.contacts) + [s["frame"] for s in model.sensors["ImuSensor"]]
    K = len(names)
    out = {"metric": "frame kinematics", "envs": B, "frames": names, "calls": args.calls, "reps": args.reps}
    for dtype in (torch.float64, torch.float32):
        eng = BatchedEngine(model, B, dtype=dtype, device=dev)
        eng.set_options({"contacts": {"model": "spring_damper"}})
        q0 = torch.as_tensor(model.neutral(), dtype=dtype, device=dev)[:, None].expand(-1, B).contiguous()
        q0[2] += 1.0
        eng.start(q0, 0.1 * torch.randn((model.nv, B), dtype=dtype, device=dev))
        pose_only = blocks.FrameKinematics(eng, names, compute_velocity=False)
        full = blocks.FrameKinematics(eng, names, compute_rpy=True, average=True,
                                      reference_frames=["ODOMETRY"] + ["LOCAL_WORLD_ALIGNED"] * (K - 1))
        full.reset()
        size = torch.finfo(dtype).bits // 8
        nq, nv = model.nq, model.nv
        lines = {
            "kinematics_pose": (pose_only.refresh, nq + 7 * K),
            "kinematics_pose_rpy_velocity": (full.refresh, nq + nv + 16 * K),
            "kinematics_reset": (full.reset, nq + nv + 23 * K),
            "average": (lambda: full.refresh_average(0.04), 14 * K + 24 * K),
        }
        samples = {k: [] for k in lines}
        for _ in range(args.reps):       # (interleaved: a drift of the clocks touches every line alike)
            for k, (fn, _) in lines.items():
                samples[k].append(timed(fn, args.calls))
        res = {}
        for k, (_, rows) in lines.items():
            nbytes = rows * size * B
            res[k] = {"median_us": round(statistics.median(samples[k]), 2), "min_us": round(min(samples[k]), 2),
                      "max_us": round(max(samples[k]), 2), "bytes": nbytes, "hbm_us": round(1e6 * nbytes / HBM_BYTES_PER_S, 2)}
        out[str(dtype).split(".")[-1]] = res
        eng.stop()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
