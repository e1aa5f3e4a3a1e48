"""Reference-pinned fixtures of the actuated-joint quantities block: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_locomotion_fixtures.py: this script parses the reference files where they lie, takes
the definitions named in SOURCES (decorators included) and executes them with `numba.jit` stubbed to the identity.  Beyond
the single names of that loader it takes a class (`EnergyGenerationMode`) and a tuple assignment (`_CHARGE, _LOST_EACH,
_LOST_GLOBAL, _PENALIZE = ...`, named by its first target), which `compute_power` reads.  Nothing of the reference is copied into
the repository: only authored descriptions, seeded inputs and the outputs the reference's code produced for them, written to
tests/golden/ref_actuation.npz.

Run where the reference tree is available:   python tools/make_ref_actuation_fixtures.py [output.npz]
                                             python tools/make_ref_actuation_fixtures.py --check     (regenerate and compare)

Tier A for the functions, a restated composition for the glue: `compute_power`, `mean` / `_mean`, `radial_basis_function` and
`CUTOFF_ESP` are the reference's, called on the arrays they are written for, one lane at a time.  What this script RESTATES, and
labels as such below: the `refresh` bodies of `MultiActuatedJointKinematic` and `_MultiActuatedJointBoundDistance`,
`MechanicalSafetyTermination.compute` (as the count of the motors its two `any` run over), the wrapping-array branch of
`StackedQuantity.refresh` and the `max_stack` formula.

A case is a sequence of launches ("events") on 64 lanes: event 0 restarts every window, a later event pushes one environment
step on every lane or restarts the windows of some lanes (what `reset_lanes` does).  `v` and `command` are drawn per event; `q`
and `a`, and the four outputs that follow them alone, are the same for every event of a case (the file stays below 500 kB).
`expected.*` holds the tensors of the block after every event: a lane an event leaves out keeps what it had.

Drawing conditions, asserted here: outside `thresholds` every pair the safety test compares is at least 1e-3 apart; the
argument of the radial basis function `average^2 / cutoff^2 <= 4`; the propagated float64 bound of the reward row
(tests/actuation_numpy.py) is at most 2.5e-14 on every lane and event (the cutoff of a case is the smallest of a geometric
ladder that meets the last two).
"""
from __future__ import annotations

import ast
import math
import os
import sys
import tempfile
import types
import typing
from enum import IntEnum

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from tests import actuation_numpy as an     # noqa: E402  (the derived bounds of the drawing conditions)

REF = os.environ.get("JIMINY_REFERENCE", "/root/reference")
COMMON = os.path.join(REF, "python/gym_jiminy/common/gym_jiminy/common")
OUT = os.path.join(HERE, "..", "tests", "golden", "ref_actuation.npz")

SOURCES = {
    "quantities/generic.py": ("EnergyGenerationMode", "compute_power", "_CHARGE"),
    "utils/math.py": ("_mean", "mean"),
    "compositions/mixin.py": ("CUTOFF_ESP", "radial_basis_function"),
}
B = 64
SEED = 20261019
EPS = float(np.finfo(np.float64).eps)
RESTART, PUSH = 0, 1
APART = 1e-3
REWARD_BOUND_MAX = 2.5e-14


def load_reference_functions() -> dict:
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    ns: dict = {"np": np, "nb": nb, "math": math, "IntEnum": IntEnum, "ArrayOrScalar": typing.Any}
    ns.update({k: getattr(typing, k) for k in ("Optional", "Tuple", "Union", "List", "Sequence", "Dict", "Literal", "overload",
                                               "no_type_check")})
    for rel, names in SOURCES.items():
        path = os.path.join(COMMON, rel)
        with open(path) as f:
            tree = ast.parse(f.read(), filename=path)
        found = set()
        for node in tree.body:
            name = None
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
                name = node.name
            elif isinstance(node, ast.Assign) and len(node.targets) == 1:
                target = node.targets[0]
                first = target.elts[0] if isinstance(target, ast.Tuple) and target.elts else target
                if isinstance(first, ast.Name) and first.id in names:
                    name = first.id
            if name is not None:      # (typing overloads first, the definition last)
                exec(compile(ast.Module([node], []), path, "exec"), ns)
                found.add(name)
        if set(names) - found:
            raise RuntimeError(f"{rel}: {sorted(set(names) - found)} not found")
    return ns


# ------------------------------------------------------------------------------------------------------ restated glue
def stack_length(horizon: float, step_dt: float) -> int:
    """RESTATED: `AverageMechanicalPowerConsumption.__init__` (quantities/generic.py:1865)."""
    return max(int(np.ceil(horizon / step_dt)), 1) + 1


def actuated_kinematic(data: np.ndarray, indices, ratios: np.ndarray, is_motor_side: bool) -> np.ndarray:
    """RESTATED: `MultiActuatedJointKinematic.refresh` (quantities/generic.py:1675-1691), the branch that gathers."""
    out = np.full((len(indices),), float("nan"))
    data.take(indices, None, out, "clip")
    if is_motor_side:
        out *= ratios
    return out


def lane_event(ref: dict, plan: dict, lane: dict, stack: dict, mode: int) -> dict:
    """One refresh of every quantity for one lane.  `stack`: `data [max_stack]` and `num_steps` of the lane's
    `StackedQuantity`, updated in place."""
    iq, iv, ratios = list(map(int, plan["idx_q"])), list(map(int, plan["idx_v"])), np.asarray(plan["reduction"], dtype=np.float64)
    side = bool(plan["motor_side"])
    out = {"position": actuated_kinematic(lane["q"], iq, ratios, side), "velocity": actuated_kinematic(lane["v"], iv, ratios, side),
           "acceleration": actuated_kinematic(lane["a"], iv, ratios, side)}
    # RESTATED: `_MultiActuatedJointBoundDistance.refresh` (compositions/generic.py:500-502), joint side
    position = actuated_kinematic(lane["q"], iq, ratios, False)
    out["bound_low"], out["bound_high"] = position - plan["position_low"], plan["position_high"] - position
    # RESTATED: `MechanicalSafetyTermination.compute` (compositions/generic.py:585-595): the motors its two `any` run over
    velocity = actuated_kinematic(lane["v"], iv, ratios, False)
    hits = ((out["bound_low"] < plan["position_margin"]) & (velocity < - plan["velocity_max"])) | \
           ((out["bound_high"] < plan["position_margin"]) & (velocity > plan["velocity_max"]))
    out["safety"] = np.int32(np.sum(hits))
    out["pairs"] = np.concatenate([out["bound_low"] - plan["position_margin"], out["bound_high"] - plan["position_margin"],
                                   velocity + plan["velocity_max"], velocity - plan["velocity_max"]])
    # the reference's `compute_power` on the motor-side velocities (`MechanicalPowerConsumption`, quantities/generic.py:1794-1805)
    power = float(ref["compute_power"](int(plan["generator_mode"]), actuated_kinematic(lane["v"], iv, ratios, True), lane["command"].copy()))
    # RESTATED: `StackedQuantity.refresh`, `is_wrapping=True, as_array=True` (quantities/transform.py:226-246, 292)
    max_stack = int(plan["max_stack"])
    num_steps = 0 if mode == RESTART else stack["num_steps"] + 1
    data = stack["data"]
    num_stack = num_steps + 1
    if num_stack < max_stack:
        data = stack["data"][..., :num_stack]
    index = num_steps % max_stack
    data[..., index] = power
    stack["num_steps"] = num_steps
    # the reference's `mean` (`AverageMechanicalPowerConsumption.refresh`, quantities/generic.py:1886-1887) and its
    # `radial_basis_function` (`MinimizeMechanicalPowerConsumption`, compositions/generic.py:186-189)
    average = float(ref["mean"](data))
    out["scalars"] = np.array([power, average, float(ref["radial_basis_function"](average, float(plan["power_cutoff"]), 2))])
    return out


def run_case(ref: dict, plan: dict, inputs: dict, modes, masks, check_pairs: bool = True) -> dict:
    """Every event of a case, lane by lane, with the carry-over of the lanes an event leaves out."""
    S = int(plan["max_stack"])
    stacks = [{"data": np.zeros(S), "num_steps": 0} for _ in range(B)]
    held: dict = {}
    rows = []
    for e, (mode, mask) in enumerate(zip(modes, masks)):
        for b in np.flatnonzero(mask):
            lane = {"q": inputs["q"][:, b].copy(), "a": inputs["a"][:, b].copy(), "v": inputs["v"][e][:, b].copy(),
                    "command": inputs["command"][e][:, b].copy()}
            got = lane_event(ref, plan, lane, stacks[b], int(mode))
            if check_pairs:
                assert np.abs(got.pop("pairs")).min() >= APART
            for k in an.OUTPUTS:
                held.setdefault(k, np.zeros((*np.shape(got[k]), B), dtype=np.asarray(got[k]).dtype))[..., b] = got[k]
        row = {k: v.copy() for k, v in held.items()}
        row["power_ring"] = np.stack([s["data"] for s in stacks], -1)
        row["power_count"] = np.array([s["num_steps"] for s in stacks], dtype=np.int32)
        rows.append(row)
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    for k in an.CONSTANT_OUTPUTS:
        assert all(np.array_equal(out[k][0], out[k][e]) for e in range(len(rows)))
        out[k] = out[k][0]
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def draw_plan(rg: np.random.Generator, M: int, S: int, generator_mode: int, motor_side: bool) -> dict:
    """Motors not in joint order (a permutation behind two leading rows of `q` and one of `v`), reductions away from 1."""
    order = rg.permutation(M)
    return dict(idx_q=(2 + order).astype(np.int32), idx_v=(1 + order).astype(np.int32), reduction=rg.uniform(20.0, 100.0, M),
                position_low=rg.uniform(-2.0, -1.0, M), position_high=rg.uniform(1.0, 2.0, M), nq=M + 2, nv=M + 1,
                generator_mode=generator_mode, max_stack=S, motor_side=motor_side, position_margin=0.4, velocity_max=0.5, power_cutoff=1.0)


def draw_inputs(rg: np.random.Generator, plan: dict, E: int, negative_lanes=None) -> dict:
    """`q` inside the bounds, `v` in [-2, 2], efforts up to 30 that mostly push along the velocity (so that the mean power is
    of the size of the sum of the magnitudes) with one in five against it; on `negative_lanes` every effort brakes."""
    M, nq, nv = len(plan["idx_q"]), int(plan["nq"]), int(plan["nv"])
    iq, iv = plan["idx_q"].astype(int), plan["idx_v"].astype(int)
    q, a = rg.uniform(-1.0, 1.0, (nq, B)), rg.uniform(-50.0, 50.0, (nv, B))
    v = rg.uniform(-2.0, 2.0, (E, nv, B))
    low, high, margin, vmax = plan["position_low"][:, None], plan["position_high"][:, None], plan["position_margin"], plan["velocity_max"]
    q[iq] = rg.uniform(low, high, (M, B))
    while True:     # every pair the safety test compares at least 1e-3 apart (with room for the test above)
        near = (np.abs(q[iq] - low - margin) < 2 * APART) | (np.abs(high - q[iq] - margin) < 2 * APART)
        if not near.any():
            break
        q[iq] = np.where(near, rg.uniform(low, high, (M, B)), q[iq])
    while True:
        near = np.abs(np.abs(v) - vmax) < 2 * APART
        if not near.any():
            break
        v = np.where(near, rg.uniform(-2.0, 2.0, v.shape), v)
    along = np.where(rg.uniform(size=(E, M, B)) < 0.8, 1.0, -1.0) * np.sign(v[:, iv])
    command = rg.uniform(1.0, 30.0, (E, M, B)) * along
    if negative_lanes is not None:
        command[..., negative_lanes] = -(np.abs(command) * np.sign(v[:, iv]))[..., negative_lanes]
    return dict(q=q, v=v, a=a, command=command)


def settle_cutoff(ref: dict, plan: dict, inputs: dict, modes, masks) -> dict:
    """The expected tensors of a case under the smallest cutoff of the ladder 1, 1.25, ... (times the largest |average|)
    that meets the drawing conditions of the reward row."""
    probe = run_case(ref, plan, inputs, modes, masks)
    scale = float(np.abs(probe["scalars"][:, an.POWER_AVERAGE]).max())
    assert scale > 0.0
    for k in range(64):
        plan["power_cutoff"] = scale * 0.5 * 1.25 ** k
        expected = run_case(ref, plan, inputs, modes, masks)
        bounds = an.scalar_bounds(plan, inputs, modes, masks, expected["scalars"], EPS)
        ratio = (expected["scalars"][:, an.POWER_AVERAGE] / plan["power_cutoff"]) ** 2
        if ratio.max() <= 4.0 and bounds[:, an.REWARD_POWER].max() <= REWARD_BOUND_MAX:
            return expected
    raise AssertionError("no cutoff meets the drawing conditions")


def pack_case(plan: dict, inputs: dict, modes, masks, expected: dict, only=None) -> dict:
    case = {f"plan.{k}": np.asarray(v) for k, v in plan.items()}
    case.update(inputs)
    case.update(mode=np.asarray(modes, dtype=np.int32), mask=np.asarray(masks, dtype=bool))
    case.update({f"expected.{k}": v for k, v in expected.items()})
    return case if only is None else {k: case[k] for k in only}


def all_lanes(E: int):
    return [RESTART] + [PUSH] * (E - 1), np.ones((E, B), dtype=bool)


def make_cases(ref: dict, rg: np.random.Generator) -> dict:
    out: dict = {}
    # regular: 12 motors, motor side, a window of 3 and 8 pushes: the ring wraps twice
    plan = draw_plan(rg, 12, 3, an.CHARGE, True)
    modes, masks = all_lanes(9)
    inputs = draw_inputs(rg, plan, 9)
    expected = settle_cutoff(ref, plan, inputs, modes, masks)
    assert expected["power_count"][-1].min() == 8 and (expected["safety"] > 0).any() and (expected["safety"] == 0).any()
    assert (an.motor_powers(plan, an.event_inputs(inputs, 1)) < 0).any()
    out["regular"] = pack_case(plan, inputs, modes, masks, expected)
    # one motor, the smallest window
    plan = draw_plan(rg, 1, stack_length(0.005, 0.01), an.PENALIZE, False)
    assert plan["max_stack"] == 2
    modes, masks = all_lanes(4)
    inputs = draw_inputs(rg, plan, 4)
    out["one_motor"] = pack_case(plan, inputs, modes, masks, settle_cutoff(ref, plan, inputs, modes, masks))
    # one case per generator mode on the same draws; every fourth lane generates on the whole
    plan = draw_plan(rg, 5, 3, an.CHARGE, False)
    modes, masks = all_lanes(4)
    negative = np.arange(B) % 4 == 0
    inputs = draw_inputs(rg, plan, 4, negative)
    for label, mode in (("charge", an.CHARGE), ("lost_each", an.LOST_EACH), ("lost_global", an.LOST_GLOBAL), ("penalize", an.PENALIZE)):
        plan = dict(plan, generator_mode=mode)
        expected = settle_cutoff(ref, plan, inputs, modes, masks)
        if mode == an.CHARGE:
            assert (an.motor_powers(plan, an.event_inputs(inputs, 0)) < 0).any(1).all()
            assert (expected["scalars"][:, an.POWER][:, negative] < 0).all() and (expected["scalars"][:, an.POWER][:, ~negative] > 0).any()
            out[label] = pack_case(plan, inputs, modes, masks, expected)
        else:
            if mode == an.LOST_GLOBAL:
                assert (expected["scalars"][:, an.POWER][:, negative] == 0).all()
            out[label] = pack_case(plan, inputs, modes, masks, expected,
                                   only=("plan.generator_mode", "plan.power_cutoff", "expected.scalars", "expected.power_ring"))
            out[label]["base"] = np.array("charge")
    # staggered: another subset of lanes restarted before each of 6 pushes
    plan = draw_plan(rg, 2, 3, an.CHARGE, False)
    modes, masks = [RESTART], [np.ones(B, dtype=bool)]
    for _ in range(6):
        subset = rg.uniform(size=B) < 0.3
        assert subset.any() and not subset.all()
        modes += [RESTART, PUSH]
        masks += [subset, np.ones(B, dtype=bool)]
    masks = np.stack(masks)
    inputs = draw_inputs(rg, plan, len(modes))
    expected = settle_cutoff(ref, plan, inputs, modes, masks)
    assert len(np.unique(expected["power_count"][-1])) >= 4
    out["staggered"] = pack_case(plan, inputs, modes, masks, expected)
    # thresholds: short binary fractions, exact in float32.  Motor 0 of lane b is of kind b % 8: kinds 0-3 sit exactly on a
    # threshold (must not count), kinds 4-7 one float32 step inside (must count); motor 2 of the lanes b % 16 >= 8 is well
    # inside and counts as well; the other motors are far from every threshold
    M = 4
    plan = dict(idx_q=np.array([2, 0, 3, 1], dtype=np.int32), idx_v=np.array([2, 0, 3, 1], dtype=np.int32), reduction=np.array([2.0, 0.5, 4.0, 8.0]),
                position_low=np.full(M, -1.0), position_high=np.full(M, 1.5), nq=M, nv=M, generator_mode=an.CHARGE, max_stack=2,
                motor_side=False, position_margin=0.25, velocity_max=0.5, power_cutoff=1.0)
    f32 = np.float32
    up = lambda x: float(np.nextafter(f32(x), f32(np.inf)))       # noqa: E731
    down = lambda x: float(np.nextafter(f32(x), f32(-np.inf)))    # noqa: E731
    kinds = [(-0.75, -1.0), (-0.875, -0.5), (1.25, 1.0), (1.375, 0.5),                          # on a threshold
             (down(-0.75), -1.0), (-0.875, down(-0.5)), (up(1.25), 1.0), (1.375, up(0.5))]     # one step inside
    q, v = np.zeros((M, B)), np.zeros((M, B))
    q[[0, 1]] = rg.integers(-32, 33, (2, B)) / 64.0           # motors 1 and 3: mid range
    v[[0, 1]] = rg.integers(-128, 129, (2, B)) / 64.0
    for b in range(B):
        q[2, b], v[2, b] = kinds[b % 8]
        q[3, b], v[3, b] = (-0.9375, -1.5) if b % 16 >= 8 else (0.125, 1.5)
    modes, masks = all_lanes(2)
    inputs = dict(q=q, v=np.stack([v, v]), a=rg.integers(-256, 257, (M, B)) / 8.0, command=rg.integers(-64, 65, (2, M, B)) / 4.0)
    for k in ("q", "v", "a", "command"):
        assert np.array_equal(inputs[k], inputs[k].astype(f32).astype(np.float64))
    plan["power_cutoff"] = 1.0
    probe = run_case(ref, plan, inputs, modes, masks, check_pairs=False)
    plan["power_cutoff"] = float(2.0 ** math.ceil(math.log2(16.0 * np.abs(probe["scalars"][:, an.POWER_AVERAGE]).max())))
    expected = run_case(ref, plan, inputs, modes, masks, check_pairs=False)
    assert an.scalar_bounds(plan, inputs, modes, masks, expected["scalars"], EPS)[:, an.REWARD_POWER].max() <= REWARD_BOUND_MAX
    lane = np.arange(B)
    assert np.array_equal(expected["safety"][0], (lane % 8 >= 4).astype(np.int32) + (lane % 16 >= 8))
    assert (expected["bound_low"][0][lane % 8 == 0] == 0.25).all() and (expected["bound_high"][0][lane % 8 == 2] == 0.25).all()
    out["thresholds"] = pack_case(plan, inputs, modes, masks, expected)
    out["thresholds"]["designed_on"] = lane % 8 < 4
    return out


def main(out_path: str, verbose: bool = True) -> None:
    ref = load_reference_functions()
    assert [stack_length(*p) for p in ((0.2, 0.01), (0.07, 0.01), (0.3, 0.1), (0.005, 0.01))] == [21, 9, 4, 2]
    rg = np.random.default_rng(SEED)
    out: dict = {}
    cases = make_cases(ref, rg)
    for label, case in cases.items():
        for k, v in case.items():
            out[f"{label}.{k}"] = v
    out["cases"] = np.array(list(cases))
    out["tier"] = np.array("A: the reference's compute_power, mean and radial_basis_function on the arrays they are written for; the "
                           "refresh bodies of the quantity classes, the safety count, the wrapping stack and max_stack are restated")
    np.savez_compressed(out_path, **out)
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if not os.path.isdir(COMMON):
        sys.exit(f"{COMMON} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            fresh = os.path.join(tmp, "ref_actuation.npz")
            main(fresh, verbose=False)
            same = open(fresh, "rb").read() == open(OUT, "rb").read()
        print("tests/golden/ref_actuation.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
