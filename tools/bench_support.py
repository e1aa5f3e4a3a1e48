#!/usr/bin/env python
"""Cost of the projected support polygon block (`jm_block_support_polygon`, `k_support_polygon`) on ANYmal (4 contact points)
and on 16 contact points of Atlas (the outer collision box of each foot: the built-in Atlas has 32 contact points, over the
kernel's bound of 16, so `blocks.SupportPolygon` refuses it and the plan is made by hand here).
    python tools/bench_support.py [--envs 65536] [--biped-envs 32768] [--calls 200] [--reps 5]
`--calls` back-to-back launches between two device events, `--reps` repetitions in one process (median, min, max in
microseconds per launch), float64, in both reference frames: the block with every output and the reward row, next to the launch
of the locomotion quantities block on the same tensors (`jm_block_locomotion`: the yardstick, the same inputs and one lane per
environment), interleaved.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jiminy_amd import _abi, blocks, load_builtin, support  # noqa: E402
from jiminy_amd.engine import BatchedEngine  # noqa: E402


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


class RawSupport:
    """A plan over chosen columns of a frame kinematics block, launched through the C ABI on the tensors of the two blocks."""

    def __init__(self, eng, fk, lq, columns, frame: int) -> None:
        self.eng, self.lib = eng, eng._lib
        desc, keep = support.make_desc(point_column=columns, n_frames=len(fk.frame_names), reference_frame=frame)
        self.h = C.c_void_p()
        with torch.cuda.device(eng.device):
            self.lib.check(self.lib.L.jm_support_plan_create(C.byref(desc), C.byref(self.h)))
        B = eng.batch_size
        new = lambda *shape, dtype=torch.float64: torch.zeros((*shape, B), dtype=dtype, device=eng.device)      # noqa: E731
        self.out = dict(n_vertices=new(dtype=torch.int32), vertex_index=new(16, dtype=torch.int32), vertices=new(2, 16), center=new(2),
                        scalars=new(2))
        self.io = _abi.SupportIO()
        self.io.pose, self.io.odom_pose, self.io.zmp = fk.pose.data_ptr(), lq.odom_pose.data_ptr(), lq.zmp.data_ptr()
        for k, t in self.out.items():
            setattr(self.io, k, t.data_ptr())

    def refresh(self) -> None:
        self.lib.check(self.lib.L.jm_block_support_polygon(self.h, _abi.JM_F64, self.eng.batch_size, C.byref(self.io), 0.05, 0.1,
                                                           self.eng._stream()))

    def close(self) -> None:
        self.lib.L.jm_support_plan_destroy(self.h)


def kernels(model, B: int, dev, calls: int, reps: int, columns_of) -> dict:
    eng = BatchedEngine(model, B, dtype=torch.float64, device=dev)
    eng.set_options({"stepper": {"odeSolver": "euler_explicit", "dtMax": 1e-3, "controllerUpdatePeriod": 1e-3,
                                 "sensorsUpdatePeriod": 1e-3}, "contacts": {"model": "constraint"}})
    eng.enable_output("centroidal")
    q0 = torch.as_tensor(model.neutral(), dtype=torch.float64, device=dev)[:, None].expand(-1, B).contiguous()
    eng.start(q0, torch.zeros((model.nv, B), dtype=torch.float64, device=dev))
    for _ in range(5):
        eng.step(1e-3)
    fk = blocks.FrameKinematics(eng, ["root_joint"] + list(model.contacts), compute_velocity=False)
    fk.reset()
    result, lines, raws = {}, {}, []
    for frame, label in ((support.odometry_frame("LOCAL_WORLD_ALIGNED"), "lwa"), (support.odometry_frame("LOCAL"), "local")):
        lq = blocks.LocomotionQuantities(eng, fk, zmp_reference_frame=frame, momentum=False)
        lq.reset()
        raw = RawSupport(eng, fk, lq, columns_of(fk), frame)
        raw.refresh()
        torch.cuda.synchronize()
        raws.append((raw, lq))
        result[f"n_vertices_{label}"] = sorted(set(raw.out["n_vertices"].cpu().tolist()))
        result[f"margin_{label}"] = [round(float(raw.out["scalars"][0].min()), 4), round(float(raw.out["scalars"][0].max()), 4)]
        lines[f"k_support_polygon_{label}"] = raw.refresh
        lines[f"k_locomotion_{label}"] = lq.refresh
    samples = {k: [] for k in lines}
    for _ in range(reps):       # (interleaved: a drift of the clocks touches every line alike)
        for k, fn in lines.items():
            samples[k].append(timed(fn, calls))
    for raw, _ in raws:
        raw.close()
    eng.stop()
    n = len(columns_of(fk))
    # a lane reads its 2 n coordinates (again and again, from cache), the odometry pose and the ZMP, and writes every output
    result.update(n_points=n, envs=B, bytes_per_lane_once=8 * (2 * n + 3 + 2) + 4 * 17 + 8 * (32 + 2 + 2),
                  **{k + "_us": summary(v) for k, v in samples.items()})
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--biped-envs", type=int, default=32768)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"metric": "projected support polygon", "calls": args.calls, "reps": args.reps}
    anymal, atlas = load_builtin("anymal"), load_builtin("atlas")
    out["anymal"] = kernels(anymal, args.envs, dev, args.calls, args.reps, lambda fk: [fk.index(c) for c in anymal.contacts])
    # the outer collision box of each foot: the contact points `*_CollisionBox_0_*`
    outer = [c for c in atlas.contacts if "_CollisionBox_0_" in c]
    assert len(outer) == 16
    out["atlas_outer_boxes"] = kernels(atlas, args.biped_envs, dev, args.calls, args.reps, lambda fk: [fk.index(c) for c in outer])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
