#!/usr/bin/env python
"""Cost of the height-map ground on the one-robot-per-lane constraint kernel: ms per step launch of
`k_constrained<double, Topo, true>` (per-lane body parameters bound, so that both runs take that instantiation) on flat
ground and on a bumpy map with a patch per lane.  One JSON line per ground, then the ratio.

    python tools/bench_lane_ground.py [--robot anymal_held] [--batch 16384] [--steps 200] [--warmup 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jiminy_amd import _abi, codegen  # noqa: E402
from jiminy_amd.engine import BatchedEngine  # noqa: E402
from jiminy_amd.randomization import sample_model_lane  # noqa: E402
from jiminy_amd.synthetic import sample_standing_states  # noqa: E402
from tests import robots  # noqa: E402


def run(model, B, steps, warmup, dt, ground):
    dev = torch.device("cuda", 0)
    st = sample_standing_states(model, B, seed=1)
    eng = BatchedEngine(model, B, dtype=torch.float64, device=dev)
    eng.set_options({"stepper": {"odeSolver": "euler_explicit", "dtMax": dt, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt},
                     "contacts": {"model": "constraint"}})
    eng.set_lane_model(sample_model_lane(model, B, {"massBodiesBiasStd": 0.05}, torch.Generator().manual_seed(1)))
    if ground:
        rg = np.random.default_rng(2)
        eng.set_ground_heightmap(0.005 * rg.standard_normal((41, 41)), -2.0, -2.0, 0.1, 0.1)
        eng.set_ground_offsets(torch.from_numpy(rg.uniform(-1.0, 1.0, (B, 2))))
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    for _ in range(warmup):
        eng.step(dt)
    torch.cuda.synchronize()
    eng.enable_timing(True)
    eng.timing_summary()
    for _ in range(steps):
        eng.step(dt)
    torch.cuda.synchronize()
    n, ms = eng.timing_summary()
    status = eng.status
    nb = _abi.constraint_rows(model)["n_bounds"]
    flags = eng.field("con_flags")[nb:nb + len(model.contacts)]
    return {"ground": "bumpy map" if ground else "flat", "robot": model.name, "batch": B, "launches": n,
            "ms_per_launch": ms / max(n, 1), "contacts_active_per_lane": float((flags & 1).sum().item()) / B,
            "lanes_nan": ((status & _abi.JM_LANE_NAN) != 0).double().mean().item()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="anymal_held")
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dt", type=float, default=1e-3)
    args = ap.parse_args()
    model = getattr(robots, args.robot)()
    assert codegen.quad_structure(model) is None, "a robot of the one-robot-per-lane family"
    flat = run(model, args.batch, args.steps, args.warmup, args.dt, False)
    print(json.dumps(flat), flush=True)
    bumpy = run(model, args.batch, args.steps, args.warmup, args.dt, True)
    print(json.dumps(bumpy), flush=True)
    print(json.dumps({"metric": "bumpy / flat ms per launch", "value": bumpy["ms_per_launch"] / flat["ms_per_launch"]}))


if __name__ == "__main__":
    main()
