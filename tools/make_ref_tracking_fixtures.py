"""Reference-pinned fixtures of the tracking windows block: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_actuation_fixtures.py (its loader is used as it is, with the SOURCES below): the
reference files are parsed where they lie, the definitions named in SOURCES are executed with `numba.jit` stubbed to the
identity.  Nothing of the reference is copied into the repository: only authored plans, seeded inputs and the outputs the
reference's code produced for them, written to tests/golden/ref_tracking.npz.

Run where the reference tree is available:   python tools/make_ref_tracking_fixtures.py [output.npz]
                                             python tools/make_ref_tracking_fixtures.py --check     (regenerate and compare)

Tier A for the functions, a restated composition for the glue: `angle_difference`, `angle_distance`, `min_norm`,
`compute_drift_error`, `l2_norm`, `quat_to_yaw` / `quat_to_yaw_cos_sin`, `radial_basis_function` and `CUTOFF_ESP` are the
reference's, called on the arrays they are written for, one lane at a time.  What this script RESTATES, and labels as such
below: both branches of `StackedQuantity.refresh`, `DeltaQuantity`, the `max_stack` formula and the composition of the five
terminations and of the reward out of them.

A case is a sequence of launches ("events") on 64 lanes: event 0 restarts every lane, a later event pushes one environment
step on every lane or restarts some lanes (what `reset_lanes` does).  Every input is drawn per event, on a grid of 2^-12
(exact in float32 too, and the file stays below 500 kB).  `expected.*` holds the tensors and the state of the block after
every event: a lane an event leaves out keeps what it had.  The state is the block's: the rings of the two shift families
hold, per timestamp, the sum of squares `min_norm` takes its minimum of; `odom_ring` holds the values of the reference's list
at slot `num_steps % max_stack`; a slot that a restart puts out of use keeps its value (the reference allocates a fresh array,
of which it shows the slots in use only).

Designed lanes (asserted in `check_designed`): lane 0 / 1 turn by +2.5 / -2.5 rad per step, through +-pi, more than a full turn
inside the window of the case `long`; lane 2 tracks its reference exactly: drift and shift 0, reward 1; lane 3 reads NaN at
event 1 of `regular`, which later leaves every window; the case `staggered` restarts lanes while the others are mid-window.
Drawing conditions, asserted here: outside lanes 0-2 every argument of `floor` is at least 1e-3 from an integer; the argument
of the radial basis function is at most 4.
"""
from __future__ import annotations

import math
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from tests import tracking_numpy as tn                  # noqa: E402  (names and layouts)
from tools import make_ref_actuation_fixtures as loader  # noqa: E402  (the loader mechanism)

COMMON = loader.COMMON
OUT = os.path.join(HERE, "..", "tests", "golden", "ref_tracking.npz")

SOURCES = {
    "utils/math.py": ("quat_to_yaw_cos_sin", "quat_to_yaw"),
    "quantities/locomotion.py": ("angle_difference",),
    "compositions/mixin.py": ("CUTOFF_ESP", "radial_basis_function"),
    "compositions/generic.py": ("compute_drift_error", "min_norm"),
    "compositions/locomotion.py": ("l2_norm", "angle_distance"),
}
B = 64
SEED = 20261020
GRID = 4096.0
RESTART, PUSH = 0, 1
APART = 1e-3
WRAP_UP, WRAP_DOWN, EQUAL, NAN_LANE = 0, 1, 2, 3
TURN = 2.5


def load_reference_functions() -> dict:
    saved, loader.SOURCES = loader.SOURCES, SOURCES
    try:
        return loader.load_reference_functions()
    finally:
        loader.SOURCES = saved


# ------------------------------------------------------------------------------------------------------ restated glue
def stack_length(horizon: float, step_dt: float) -> int:
    """RESTATED: quantities/locomotion.py:1572-1573, compositions/generic.py:429-430."""
    assert horizon >= step_dt
    return max(int(np.ceil(horizon / step_dt)), 1) + 1


class Stacked:
    """RESTATED: `StackedQuantity` (quantities/transform.py:180-301) of one lane: `initialize` at a restart, `refresh` with the
    simulation running, `as_array` with or without wrapping, and the list with `is_wrapping=False` that `DeltaQuantity` reads."""

    def __init__(self, max_stack: int, is_wrapping: bool, as_array: bool) -> None:
        self.max_stack, self.is_wrapping, self.as_array = max_stack, is_wrapping, as_array
        self.data, self.values, self.num_steps = None, [], -1

    def restart(self, value: np.ndarray) -> None:
        self.values = []
        if self.as_array:
            self.data = np.zeros((*np.shape(value), self.max_stack), order="F")
        self.num_steps = -1

    def refresh(self, value):
        self.num_steps += 1
        num_steps = self.num_steps
        if self.as_array:
            data = self.data
            num_stack = num_steps + 1
            if num_stack < self.max_stack:
                data = self.data[..., :num_stack]
        if self.is_wrapping:
            index = num_steps % self.max_stack
        is_stack_full = num_steps >= self.max_stack
        if self.as_array:
            if self.is_wrapping:
                data[..., index] = value
            else:
                if is_stack_full:
                    data[..., :-1] = data[..., 1:].copy()
                data[..., -1] = value
            return data
        assert not self.is_wrapping
        if is_stack_full:
            self.values.pop(0)
        self.values.append(np.array(value, copy=True))
        return list(self.values)


class Delta:
    """RESTATED: `DeltaQuantity` (quantities/transform.py:715-831) of one lane."""

    def __init__(self, max_stack: int, op, bounds_only: bool) -> None:
        self.op, self.bounds_only = op, bounds_only
        if bounds_only:
            self.stack = Stacked(max_stack, False, False)
        else:
            self.inner = Delta(2, op, True)
            self.stack = Stacked(max_stack - 1, True, True)

    def restart(self, value) -> None:
        if self.bounds_only:
            self.stack.restart(value)
        else:
            self.inner.restart(value)
            self.stack.restart(value)

    def refresh(self, value):
        if self.bounds_only:
            stack = self.stack.refresh(value)
            return self.op(stack[-1], stack[0])
        return self.stack.refresh(self.inner.refresh(value)).sum(axis=-1)


class Lane:
    """RESTATED: the five terminations and the reward of one lane, out of the pieces above -- what
    `DriftTrackingQuantityTermination` (compositions/generic.py:291-304), `ShiftTrackingQuantityTermination` (:433-443),
    `DriftTrackingBaseOdometryPoseReward` (compositions/locomotion.py:107-120) and `TrackingQuantityReward`
    (compositions/generic.py:64-122: the kernel of true - reference) compose."""

    def __init__(self, ref: dict, plan: dict) -> None:
        self.ref, self.plan = ref, plan
        sub = lambda a, b: a - b      # noqa: E731
        So, Sf, Sm = (int(plan[f"max_stack_{f}"]) for f in ("odom", "foot", "motor"))
        self.q: dict = {}
        for side in ("true", "ref"):
            if So:
                self.q[f"dxy_{side}"] = Delta(So, sub, True)
                self.q[f"dyaw_{side}"] = Delta(So, ref["angle_difference"], False)
            if Sf:
                self.q[f"fxy_{side}"], self.q[f"fyaw_{side}"] = Stacked(Sf, True, True), Stacked(Sf, True, True)
            if Sm:
                self.q[f"motor_{side}"] = Stacked(Sm, True, True)

    def values(self, lane: dict) -> dict:
        v: dict = {}
        for side, pre in (("true", ""), ("ref", "reference_")):
            if f"dxy_{side}" in self.q:
                pose = lane[pre + "odom_pose"]
                v[f"dxy_{side}"], v[f"dyaw_{side}"] = pose[:2].copy(), pose[2:].copy()       # (`MaskedQuantity`, keys (0, 1) / (2,))
            if f"fxy_{side}" in self.q:
                pose = lane[pre + "relative_pose"]
                v[f"fxy_{side}"] = pose[:2].copy()
                v[f"fyaw_{side}"] = self.ref["quat_to_yaw"](np.ascontiguousarray(pose[3:]))
            if f"motor_{side}" in self.q:
                v[f"motor_{side}"] = lane[pre + "position"].copy()
        return v

    def event(self, lane: dict, mode: int) -> dict:
        ref, plan, v = self.ref, self.plan, self.values(lane)
        if mode == RESTART:
            for k, q in self.q.items():
                q.restart(v[k])
        got = {k: q.refresh(v[k]) for k, q in self.q.items()}
        out = {"scalars": np.zeros(6), "floor_args": []}
        num_steps = next(iter(self.q.values()))
        num_steps = (num_steps.stack if isinstance(num_steps, Delta) else num_steps).num_steps
        out["count"] = np.int32(num_steps)
        if "dxy_true" in got:
            S = int(plan["max_stack_odom"])
            out["delta_odom"] = np.concatenate([got["dxy_true"], got["dyaw_true"]])
            out["delta_odom_reference"] = np.concatenate([got["dxy_ref"], got["dyaw_ref"]])
            out["scalars"][tn.DRIFT_POSITION] = ref["compute_drift_error"](got["dxy_true"], got["dxy_ref"])
            out["scalars"][tn.DRIFT_ORIENTATION] = ref["compute_drift_error"](got["dyaw_true"], got["dyaw_ref"])
            error = np.array([ref["l2_norm"](got["dxy_true"]), got["dyaw_true"][0]]) - \
                np.array([ref["l2_norm"](got["dxy_ref"]), got["dyaw_ref"][0]])
            out["scalars"][tn.REWARD_ODOM_POSE] = ref["radial_basis_function"](error, float(plan["odometry_cutoff"]), 2)
            out["rbf_arg"] = float(error @ error) / float(plan["odometry_cutoff"]) ** 2
            # the block's state: the list of the reference at slot num_steps % max_stack; its wrapping array as it is
            out["odom_slot"] = np.concatenate([v["dxy_true"], v["dxy_ref"]])
            out["yaw_prev"] = np.array([v["dyaw_true"][0], v["dyaw_ref"][0]])
            out["yaw_ring"] = np.stack([self.q["dyaw_true"].stack.data[0], self.q["dyaw_ref"].stack.data[0]], -1)
            assert out["yaw_ring"].shape == (S - 1, 2)
            for side in ("true", "ref"):
                inner = self.q[f"dyaw_{side}"].inner.stack.values
                out["floor_args"].append((inner[-1][0] - inner[0][0] + np.pi) / (2 * np.pi))
        if "fxy_true" in got:
            # RESTATED: `compute_min_distance` (compositions/generic.py:353) with op = sub / `angle_distance`
            diff_xy = got["fxy_true"] - got["fxy_ref"]
            diff_yaw = ref["angle_distance"](got["fyaw_true"], got["fyaw_ref"])
            out["scalars"][tn.SHIFT_FOOT_POSITIONS] = ref["min_norm"](diff_xy)
            out["scalars"][tn.SHIFT_FOOT_ORIENTATIONS] = ref["min_norm"](diff_yaw)
            out["foot_ring"] = np.stack([self.squares(self.q["fxy_true"], self.q["fxy_ref"], lambda a, b: a - b),
                                         self.squares(self.q["fyaw_true"], self.q["fyaw_ref"], ref["angle_distance"])])
            out["floor_args"] += list((v["fyaw_true"] - v["fyaw_ref"]) / (2 * np.pi))
        if "motor_true" in got:
            out["scalars"][tn.SHIFT_MOTOR_POSITIONS] = ref["min_norm"](got["motor_true"] - got["motor_ref"])
            out["motor_ring"] = self.squares(self.q["motor_true"], self.q["motor_ref"], lambda a, b: a - b)
        return out

    @staticmethod
    def squares(left: Stacked, right: Stacked, op) -> np.ndarray:
        """RESTATED: the inside of `min_norm` (compositions/generic.py:328-330) on the whole arrays of two stacks: the sum of
        squares of every timestamp, by slot (slots not written yet hold zeros)."""
        values = op(left.data, right.data)
        return np.sum(np.square(values).reshape((-1, values.shape[-1])), axis=0)


def run_case(ref: dict, plan: dict, inputs: dict, modes, masks) -> dict:
    """Every event of a case, lane by lane, with the carry-over of the lanes an event leaves out."""
    lanes = [Lane(ref, plan) for _ in range(B)]
    names = tn.OUTPUTS + tuple(n for n in tn.state_names(plan))
    held = {n: np.zeros(tn.shape(n, plan, B), dtype=tn.dtype_of(n, np.float64)) for n in names}
    rows, rbf_args, floor_args = [], [], []
    for e, (mode, mask) in enumerate(zip(modes, masks)):
        for b in np.flatnonzero(mask):
            with np.errstate(invalid="ignore"):
                got = lanes[b].event({k: v[e][..., b].copy() for k, v in inputs.items()}, int(mode))
            if "odom_slot" in got:
                held["odom_ring"][int(got["count"]) % int(plan["max_stack_odom"]), :, b] = got.pop("odom_slot")
                rbf_args.append(got.pop("rbf_arg"))
            floor_args.append((e, b, got.pop("floor_args")))
            # the block's rings: the slots in use are the reference's; the reference starts an episode on a fresh array and
            # shows `num_stack` slots of it, the block leaves the slots a restart puts out of use as they were
            for k, axis in (("yaw_ring", 0), ("foot_ring", 1), ("motor_ring", 0)):
                if k in got:
                    ring = np.moveaxis(got.pop(k), axis, 0)
                    n = min(int(got["count"]) + 1, ring.shape[0])
                    np.moveaxis(held[k][..., b], axis, 0)[:n] = ring[:n]
            for k, v in got.items():
                held[k][..., b] = v
        rows.append({k: v.copy() for k, v in held.items()})
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    # drawing conditions
    finite = [a for a in rbf_args if np.isfinite(a)]
    assert not finite or max(finite) <= 4.0, max(finite)
    for e, b, args in floor_args:
        if b not in (WRAP_UP, WRAP_DOWN, EQUAL):
            args = np.asarray([a for a in args if np.isfinite(a)])
            assert np.all(np.abs(args - np.round(args)) >= APART), (e, b, args)
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def on_grid(x):
    return np.round(np.asarray(x, dtype=np.float64) * GRID) / GRID


def wrap(yaw):
    return yaw - np.floor((yaw + np.pi) / (2 * np.pi)) * (2 * np.pi)


def draw_inputs(rg: np.random.Generator, plan: dict, E: int, nan_event=None) -> dict:
    """A random walk of the odometry pose with yaw steps of at most 1 rad kept inside [-pi, pi], the reference next to it;
    relative foot poses with full quaternions, the reference a small rotation and offset away; motor positions in [-1, 1]."""
    R, M = int(plan["n_rel"]), int(plan["n_motors"])
    inp: dict = {}
    if plan["max_stack_odom"]:
        walk = np.cumsum(rg.uniform(-0.3, 0.3, (E, 3, B)), 0) + rg.uniform(-2.0, 2.0, (1, 3, B))
        walk[:, 2] = np.cumsum(rg.uniform(-1.0, 1.0, (E, B)), 0) + rg.uniform(-np.pi, np.pi, (1, B))
        other = walk + np.cumsum(rg.uniform(-0.05, 0.05, (E, 3, B)), 0)
        for lane, sign in ((WRAP_UP, 1.0), (WRAP_DOWN, -1.0)):
            walk[:, 2, lane] = sign * (3.0 + TURN * np.arange(E))
            other[:, 2, lane] = walk[:, 2, lane] + np.cumsum(rg.uniform(-0.05, 0.05, E))
        walk[:, 2], other[:, 2] = wrap(walk[:, 2]), wrap(other[:, 2])
        inp["odom_pose"], inp["reference_odom_pose"] = on_grid(walk), on_grid(other)
    if plan["max_stack_foot"]:
        def poses():
            p = rg.uniform(-0.5, 0.5, (E, 7, R, B))
            quat = rg.normal(size=(E, 4, R, B))
            p[:, 3:] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
            return p
        def nearby(p):
            p = p + rg.uniform(-0.05, 0.05, p.shape)
            p[:, 3:] /= np.linalg.norm(p[:, 3:], axis=1, keepdims=True)
            return on_grid(p)
        rel = on_grid(poses())
        other = nearby(rel)
        while True:     # the argument of the floor of `angle_distance` away from an integer (with room for the test above)
            arg = (tn.pose_yaw(np.moveaxis(rel, 1, 0)) - tn.pose_yaw(np.moveaxis(other, 1, 0))) / (2 * np.pi)
            near = np.abs(arg - np.round(arg)) < 2 * APART
            if not near.any():
                break
            other = np.where(near[:, None], nearby(rel), other)
        inp["relative_pose"], inp["reference_relative_pose"] = rel, other
    if plan["max_stack_motor"]:
        pos = rg.uniform(-1.0, 1.0, (E, M, B))
        inp["position"], inp["reference_position"] = on_grid(pos), on_grid(pos + rg.uniform(-0.1, 0.1, pos.shape))
    for true, other in tn.FAMILY_INPUTS.values():
        if true in inp:
            inp[other][..., EQUAL] = inp[true][..., EQUAL]
            if nan_event is not None:
                inp[true][nan_event, ..., NAN_LANE] = np.nan
    for v in inp.values():
        ok = np.isfinite(v)
        assert np.array_equal(v[ok], v[ok].astype(np.float32).astype(np.float64))
    return inp


def settle_cutoff(ref: dict, plan: dict, inputs: dict, modes, masks) -> dict:
    """The expected tensors of a case under a cutoff (a power of two) at which the argument of the kernel is at most 4."""
    if not plan["max_stack_odom"]:
        return run_case(ref, plan, inputs, modes, masks)
    plan["odometry_cutoff"] = 1024.0
    probe = run_case(ref, plan, inputs, modes, masks)
    arg = -np.log(probe["scalars"][:, tn.REWARD_ODOM_POSE]) / np.log(100.0) * 1024.0 ** 2        # the squared norm of the error
    plan["odometry_cutoff"] = float(2.0 ** math.ceil(math.log2(math.sqrt(np.nanmax(arg)) / 2.0 + 1e-9)))
    return run_case(ref, plan, inputs, modes, masks)


def pack_case(plan: dict, inputs: dict, modes, masks, expected: dict) -> dict:
    case = {f"plan.{k}": np.asarray(v) for k, v in plan.items()}
    case.update(inputs)
    case.update(mode=np.asarray(modes, dtype=np.int32), mask=np.asarray(masks, dtype=bool))
    case.update({f"expected.{k}": v for k, v in expected.items()})
    return case


def all_lanes(E: int):
    return [RESTART] + [PUSH] * (E - 1), np.ones((E, B), dtype=bool)


def new_plan(So: int, Sf: int, Sm: int, R: int, M: int) -> dict:
    return dict(max_stack_odom=So, max_stack_foot=Sf, max_stack_motor=Sm, n_rel=R if Sf else 0, n_motors=M if Sm else 0,
                odometry_cutoff=0.0)


def check_designed(label: str, plan: dict, inputs: dict, expected: dict) -> None:
    sc = expected["scalars"]
    if plan["max_stack_odom"]:
        yaw = inputs["odom_pose"][:, 2]
        for lane, sign in ((WRAP_UP, 1.0), (WRAP_DOWN, -1.0)):
            jumps = np.diff(yaw[:, lane])
            assert (sign * jumps < -np.pi).any(), "the lane walks through +-pi"
            steps = sign * expected["delta_odom"][:, 2, lane]
            if label != "staggered":        # (there a lane skips the events that restart others: its turns are no multiples)
                assert np.all(steps[1:] > TURN - 1e-2), "every step is counted with its sign"
            if label == "long":
                assert steps.max() > 2 * np.pi, "more than a full turn inside the window"
        assert np.all(sc[:, [tn.DRIFT_POSITION, tn.DRIFT_ORIENTATION], EQUAL] == 0.0) and np.all(sc[:, tn.REWARD_ODOM_POSE, EQUAL] == 1.0)
    rows = [r for f in tn.families(plan) if f != "odom" for r in tn.FAMILY_ROWS[f]]
    assert np.all(sc[:, rows, EQUAL] == 0.0)
    if label == "regular":
        rows = [r for f in tn.families(plan) for r in tn.FAMILY_ROWS[f]]
        assert np.isnan(sc[1][rows, NAN_LANE]).all(), "the NaN enters every window at event 1"
        assert np.isfinite(sc[-1][:, NAN_LANE]).all() and np.isfinite(sc[-2][:, NAN_LANE]).all(), "and has left them at the end"
        assert np.isfinite(np.delete(sc, NAN_LANE, axis=-1)).all()
        for n in tn.state_names(plan):
            assert np.isfinite(expected[n][-1][..., NAN_LANE]).all()
    else:
        assert np.isfinite(sc).all()


def make_cases(ref: dict, rg: np.random.Generator) -> dict:
    out: dict = {}
    # regular: the three families on three horizons, windows of 3, 2 and 3 and 8 pushes: every ring wraps at least twice;
    # 12 motors, one relative foot; the NaN of lane 3 at event 1
    plan = new_plan(stack_length(0.08, 0.04), stack_length(0.04, 0.04), stack_length(0.07, 0.04), 1, 12)
    assert (plan["max_stack_odom"], plan["max_stack_foot"], plan["max_stack_motor"]) == (3, 2, 3)
    modes, masks = all_lanes(9)
    inputs = draw_inputs(rg, plan, 9, nan_event=1)
    expected = settle_cutoff(ref, plan, inputs, modes, masks)
    assert expected["count"][-1].min() == 8
    check_designed("regular", plan, inputs, expected)
    out["regular"] = pack_case(plan, inputs, modes, masks, expected)
    # feet: three relative feet, the smallest windows, no motor family
    plan = new_plan(2, 2, 0, 3, 0)
    modes, masks = all_lanes(5)
    inputs = draw_inputs(rg, plan, 5)
    expected = settle_cutoff(ref, plan, inputs, modes, masks)
    check_designed("feet", plan, inputs, expected)
    out["feet"] = pack_case(plan, inputs, modes, masks, expected)
    # long: windows one longer than the events: they never fill; two motors
    plan = new_plan(5, 5, 5, 1, 2)
    modes, masks = all_lanes(4)
    inputs = draw_inputs(rg, plan, 4)
    expected = settle_cutoff(ref, plan, inputs, modes, masks)
    check_designed("long", plan, inputs, expected)
    out["long"] = pack_case(plan, inputs, modes, masks, expected)
    # staggered: another subset of lanes restarted before each of 4 pushes, the others mid-window; no foot family
    plan = new_plan(3, 0, 2, 0, 2)
    modes, masks = [RESTART], [np.ones(B, dtype=bool)]
    for _ in range(4):
        subset = rg.uniform(size=B) < 0.3
        assert subset.any() and not subset.all()
        modes += [RESTART, PUSH]
        masks += [subset, np.ones(B, dtype=bool)]
    masks = np.stack(masks)
    inputs = draw_inputs(rg, plan, len(modes))
    expected = settle_cutoff(ref, plan, inputs, modes, masks)
    assert len(np.unique(expected["count"][-1])) >= 4
    check_designed("staggered", plan, inputs, expected)
    out["staggered"] = pack_case(plan, inputs, modes, masks, expected)
    return out


def main(out_path: str, verbose: bool = True) -> None:
    ref = load_reference_functions()
    assert [stack_length(*p) for p in ((1.0, 0.04), (0.04, 0.04), (0.07, 0.04), (0.3, 0.1))] == [26, 2, 3, 4]
    rg = np.random.default_rng(SEED)
    out: dict = {}
    cases = make_cases(ref, rg)
    for label, case in cases.items():
        for k, v in case.items():
            out[f"{label}.{k}"] = v
    out["cases"] = np.array(list(cases))
    out["tier"] = np.array("A: the reference's angle_difference, angle_distance, min_norm, compute_drift_error, l2_norm, quat_to_yaw and "
                           "radial_basis_function on the arrays they are written for; StackedQuantity.refresh, DeltaQuantity, max_stack "
                           "and the composition of the terminations and the reward are restated")
    np.savez_compressed(out_path, **out)
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")
    assert os.path.getsize(out_path) < 500e3


if __name__ == "__main__":
    if not os.path.isdir(COMMON):
        sys.exit(f"{COMMON} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            fresh = os.path.join(tmp, "ref_tracking.npz")
            main(fresh, verbose=False)
            same = open(fresh, "rb").read() == open(OUT, "rb").read()
        print("tests/golden/ref_tracking.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
