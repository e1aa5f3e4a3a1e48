#!/usr/bin/env python
"""The observation side of an environment step, three ways, on the ANYmal PD pipeline:

  assembled   `wrappers.AssembleObservation` (one launch of `jm_block_observe`)
  chain       the chain of tensor wrappers of the same configuration (JIMINY_AMD_TENSOR_BLOCKS=1 builds the same)
  flatten     `flatten_anymal_obs` of examples/ppo_anymal.py (`torch.cat` of strided views, `.float()`), for the plain
              configuration only, which is the one it computes

for two configurations: `plain` (the feature vector of examples/ppo_anymal.py: a layout, no scale, no stack) and `shaped` (a layout,
scales, bounds and a stack of 3).  Per variant: the tensor operations dispatched per step on top of `env.step` (counted under a
`TorchDispatchMode`, views apart), and the device-event time of whole environment steps -- the variants take turns on ONE
environment, round after round, and the median and the minimum over the rounds are printed, next to the bare `env.step`.

    python tools/bench_observe.py [--envs 4096] [--rounds 15] [--steps 20] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from jiminy_amd import wrappers as W                      # noqa: E402
from jiminy_amd.envs import make_anymal_env               # noqa: E402


def configurations() -> dict:
    from ppo_anymal import ANYMAL_OBS_LAYOUT
    shaped = dict(layout=[(("joints", "q"), ("states", "agent", "q", [(7, 19)])), (("joints", "v"), ("states", "agent", "v", [(6, 18)])),
                          (("base", "twist"), ("states", "agent", "v", [(0, 6)])), (("imu",), ("measurements", "ImuSensor")),
                          (("targets",), ("actions", "pd_controller", [0, ()]))],
                  nested_scale=[(("joints",), 2.0), (("joints", "v"), 4.0), (("base", "twist", [(3, 6)]), 8.0), (("imu",), 9.81)],
                  bounds={("joints", "q"): (-3.0, 3.0), ("targets",): (-2.0, 2.5)}, num_stack=3, nested_filter_keys=[("joints",), ("imu",)])
    return {"plain": dict(layout=ANYMAL_OBS_LAYOUT), "shaped": shaped}


class Shared:
    """One environment behind several wrappers: each wrapper steps it in its turn."""

    def __init__(self, env) -> None:
        self.env, self.engine = env, env.engine

    def __getattr__(self, name):
        return getattr(self.env, name)


def count_ops(step, inner_env, action) -> dict:
    from torch.utils._python_dispatch import TorchDispatchMode
    log, span = [], []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            log.append(func)
            return func(*args, **(kwargs or {}))
    inner = inner_env.step

    def marked(a):
        span.append(len(log))
        out = inner(a)
        span.append(len(log))
        return out
    inner_env.step = marked
    try:
        with Record():
            step(action)
    finally:
        del inner_env.step
    extra = log[:span[0]] + log[span[1]:]
    return {"all": len(extra), "not_views": sum(not f.is_view for f in extra)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_observe.py needs a HIP device")
    os.environ.pop("JIMINY_AMD_TENSOR_BLOCKS", None)
    from ppo_anymal import flatten_anymal_obs
    dev = torch.device("cuda", 0)
    env = make_anymal_env(args.envs, device=dev)
    env.reset(seed=0)
    action = torch.zeros(args.envs, env.model.nmotors, dtype=torch.float64, device=dev)
    result = {"envs": args.envs, "rounds": args.rounds, "steps_per_round": args.steps, "configurations": {}}
    for name, spec in configurations().items():
        shared = Shared(env)
        fused = W.AssembleObservation(shared, dtype=torch.float32, **spec)
        chain = fused._tensor_chain(shared)
        variants = {"env.step alone": lambda a: env.step(a), "assembled": fused.step, "chain": chain.step}
        if name == "plain":
            variants["flatten"] = lambda a: (flatten_anymal_obs(env.step(a)[0]),)
        fused.reset(seed=0)
        chain.reset(seed=0)
        out = {}
        for label, step in variants.items():
            for _ in range(3):
                step(action)
            out[label] = {"ops_on_top_of_env_step": count_ops(step, shared if label in ("assembled", "chain") else env, action)
                          if label != "env.step alone" else {"all": 0, "not_views": 0}, "ms_per_step": []}
        for _ in range(args.rounds):
            for label, step in variants.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.steps):
                    step(action)
                stop.record()
                stop.synchronize()
                out[label]["ms_per_step"].append(start.elapsed_time(stop) / args.steps)
        for label, r in out.items():
            t = r.pop("ms_per_step")
            r["median_ms"], r["min_ms"] = statistics.median(t), min(t)
            print(f"{name:7s} {label:15s} ops on top of env.step: {r['ops_on_top_of_env_step']['all']:3d} "
                  f"({r['ops_on_top_of_env_step']['not_views']:3d} not views)   step: median {r['median_ms']:.3f} ms, min {r['min_ms']:.3f} ms")
        result["configurations"][name] = out
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
