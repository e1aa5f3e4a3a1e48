"""Reference-pinned fixtures of the tracking rewards block: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_locomotion_fixtures.py: this script parses the reference files where they lie, takes
the function definitions named in SOURCES (decorators included) and the constant `CUTOFF_ESP`, and executes them with
`numba.jit` stubbed to the identity.  Nothing of the reference is copied into the repository: only authored descriptions,
seeded inputs and the outputs the reference's code produced for them, written to tests/golden/ref_tracking_rewards.npz.

Run where the reference tree is available:   python tools/make_ref_tracking_rewards_fixtures.py [output.npz]
                                             python tools/make_ref_tracking_rewards_fixtures.py --check     (regenerate and compare)

Tier A for the functions, a restated composition for the glue: `compute_height`, `quat_apply` and `radial_basis_function` (with
`CUTOFF_ESP`) are the reference's, called on the arrays they are written for, one lane at a time.  What this script RESTATES,
and labels as such below, is what surrounds them: the `refresh` of `BaseSpatialAverageVelocity` with the mask (0, 1, 5) of
`BaseOdometryAverageVelocity`, the subtraction of `BinaryOpQuantity` in `TrackingQuantityReward`, and the reads of the root and
contact columns of a pose tensor that stand for `FramePosition` / `MultiFramePosition`.

Every case holds 64 lanes; the reference side of a lane is drawn so that the error of every term is `u cutoff` with u uniform
in [0, 2]: `err^2 / cutoff^2 <= 4`.  Designed lanes (`designed_lanes` names them): `tie`, two contacts share the lowest z;
`below`, the root is below every contact and the height is negative; `zero`, the reference side is the true side and every
reward is exactly 1; `cutoff`, the error of every term is its cutoff and every reward is `CUTOFF_ESP`.
"""
from __future__ import annotations

import ast
import math
import os
import sys
import tempfile
import types
import typing

import numpy as np

REF = os.environ.get("JIMINY_REFERENCE", "/root/reference")
COMMON = os.path.join(REF, "python/gym_jiminy/common/gym_jiminy/common")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_tracking_rewards.npz")

SOURCES = {
    "utils/math.py": ("quat_apply",),
    "quantities/locomotion.py": ("compute_height",),
    "compositions/mixin.py": ("CUTOFF_ESP", "radial_basis_function"),
}
B = 64
SEED = 20261020
DESIGNED = ("tie", "below", "zero", "cutoff")
INPUTS = ("pose", "pose_reference", "v_avg", "quat_no_yaw", "v_avg_reference", "quat_no_yaw_reference", "dcm", "dcm_reference",
          "position", "position_reference")
OUTPUTS = ("value", "reference", "rewards")


def load_reference_functions() -> dict:
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    ns: dict = {"np": np, "nb": nb, "math": math, "ArrayOrScalar": typing.Any}
    ns.update({k: getattr(typing, k) for k in ("Optional", "Tuple", "Union", "List", "Sequence", "Dict", "Literal", "overload",
                                               "no_type_check")})
    for rel, names in SOURCES.items():
        path = os.path.join(COMMON, rel)
        with open(path) as f:
            tree = ast.parse(f.read(), filename=path)
        found = set()
        for node in tree.body:
            is_function = isinstance(node, ast.FunctionDef) and node.name in names
            is_constant = (isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name)
                           and node.targets[0].id in names)
            if is_function or is_constant:      # (typing overloads first, the definition last)
                exec(compile(ast.Module([node], []), path, "exec"), ns)
                found.add(node.name if is_function else node.targets[0].id)
        if set(names) - found:
            raise RuntimeError(f"{rel}: {sorted(set(names) - found)} not found")
    return ns


# ------------------------------------------------------------------------------------------------------ restated glue
def side_quantities(ref: dict, plan: dict, lane: dict, suffix: str) -> np.ndarray:
    """RESTATED reads and `refresh` bodies around the reference's own functions for one side of one lane: `BaseRelativeHeight`
    (quantities/locomotion.py:153) on the root and contact columns of `pose`; `BaseSpatialAverageVelocity` (:281-288) masked
    with (0, 1, 5) as in `BaseOdometryAverageVelocity` (:329-333); the capture point and the joint positions as they come."""
    pose = lane["pose" + suffix]
    base_pos = pose[:3, int(plan["root_column" + suffix])].copy()
    contacts_pos = np.asfortranarray(pose[:3][:, [int(k) for k in plan["contact_column" + suffix]]])
    height = float(ref["compute_height"](base_pos, contacts_pos))
    root = int(plan["root_column" + suffix])
    v_spatial = lane["v_avg" + suffix][:, root].copy()
    out_spatial = np.zeros(6)
    ref["quat_apply"](lane["quat_no_yaw" + suffix][:, root].copy(), v_spatial.reshape((2, 3)).T, out_spatial.reshape((2, 3)).T)
    return np.concatenate([[height], out_spatial[[0, 1, 5]], lane["dcm" + suffix], lane["position" + suffix]])


def lane_outputs(ref: dict, plan: dict, lane: dict) -> dict:
    """RESTATED `TrackingQuantityReward` (compositions/generic.py:113-122): the subtraction of the two sides and the
    reference's `radial_basis_function` of every term."""
    value, reference = side_quantities(ref, plan, lane, ""), side_quantities(ref, plan, lane, "_reference")
    rows = (slice(0, 1), slice(1, 4), slice(4, 6), slice(6, None))
    rewards = np.array([ref["radial_basis_function"](value[r] - reference[r], float(plan["cutoff"][k]), 2) for k, r in enumerate(rows)])
    return dict(value=value, reference=reference, rewards=rewards)


# ------------------------------------------------------------------------------------------------------------ cases
def quat_axis_angle(axis: np.ndarray, angle: float) -> np.ndarray:
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])


def random_tilt(rg: np.random.Generator) -> np.ndarray:
    axis = rg.normal(size=3)
    axis[2] = 0.0
    q = quat_axis_angle(axis / np.linalg.norm(axis), rg.uniform(-1.0, 1.0))
    return q / np.linalg.norm(q)


def random_pose(rg: np.random.Generator) -> np.ndarray:
    axis = rg.normal(size=3)
    q = quat_axis_angle(axis / np.linalg.norm(axis), rg.uniform(-np.pi, np.pi))
    return np.concatenate([rg.uniform(-2.0, 2.0, 2), rg.uniform(0.0, 1.0, 1), q / np.linalg.norm(q)])


def direction(rg: np.random.Generator, n: int) -> np.ndarray:
    d = rg.normal(size=n)
    return d / np.linalg.norm(d)


def make_case(ref: dict, rg: np.random.Generator, nc: int, n_motors: int, K: int, Kr: int) -> dict:
    columns, columns_r = rg.permutation(K), rg.permutation(Kr)
    plan = dict(n_motors=n_motors, n_frames=K, root_column=int(columns[0]), contact_column=columns[1:1 + nc].astype(np.int32),
                n_frames_reference=Kr, root_column_reference=int(columns_r[0]),
                contact_column_reference=columns_r[1:1 + nc].astype(np.int32), cutoff=rg.uniform(0.1, 1.0, 4))
    root, root_r = plan["root_column"], plan["root_column_reference"]
    col, col_r = plan["contact_column"], plan["contact_column_reference"]
    lanes = []
    for b in range(B):
        kind = DESIGNED[b] if b < len(DESIGNED) else ""
        u = np.ones(4) if kind == "cutoff" else np.zeros(4) if kind == "zero" else rg.uniform(0.0, 2.0, 4)
        err = u * plan["cutoff"]
        lane = dict(pose=np.stack([random_pose(rg) for _ in range(K)], axis=1),
                    pose_reference=np.stack([random_pose(rg) for _ in range(Kr)], axis=1),
                    v_avg=rg.uniform(-2.0, 2.0, (6, K)), v_avg_reference=rg.uniform(-2.0, 2.0, (6, Kr)),
                    quat_no_yaw=np.stack([random_tilt(rg) for _ in range(K)], axis=1),
                    quat_no_yaw_reference=np.stack([random_tilt(rg) for _ in range(Kr)], axis=1),
                    dcm=rg.uniform(-1.0, 1.0, 2), position=rg.uniform(-1.5, 1.5, n_motors))
        if kind == "tie" and nc > 1:
            lane["pose"][2, col[1]] = lane["pose"][2, col[0]] = lane["pose"][2, col].min() - 0.125
        if kind == "below":
            lane["pose"][2, root] = lane["pose"][2, col].min() - 0.25
        if kind == "zero":
            # the reference side is the true side, column by column
            for name in ("pose", "v_avg", "quat_no_yaw"):
                lane[name + "_reference"][:, root_r] = lane[name][:, root]
                lane[name + "_reference"][:, col_r] = lane[name][:, col]
        true = side_quantities(ref, plan, {**lane, "dcm_reference": lane["dcm"], "position_reference": lane["position"]}, "")
        if kind != "zero":
            # height: the root of the reference side set so that the error is `err[0]`
            sign = 1.0 if rg.uniform() < 0.5 else -1.0
            lane["pose_reference"][2, root_r] = lane["pose_reference"][2, col_r].min() + true[0] - sign * err[0]
            # velocity: the rows (0, 1, 5) of the reference side in its odometry frame, turned back into the local frame
            # (RESTATED: the inverse of `quat_apply` as the conjugate's)
            target = rg.uniform(-2.0, 2.0, 6)
            target[[0, 1, 5]] = true[1:4] - err[1] * direction(rg, 3)
            conj = lane["quat_no_yaw_reference"][:, root_r] * np.array([-1.0, -1.0, -1.0, 1.0])
            local = np.zeros(6)
            ref["quat_apply"](conj, target.reshape((2, 3)).T, local.reshape((2, 3)).T)
            lane["v_avg_reference"][:, root_r] = local
        lane["dcm_reference"] = lane["dcm"] - err[2] * direction(rg, 2)
        lane["position_reference"] = lane["position"] - err[3] * direction(rg, n_motors)
        lane["expected"] = lane_outputs(ref, plan, lane)
        e = lane["expected"]
        rows = (slice(0, 1), slice(1, 4), slice(4, 6), slice(6, None))
        for k, r in enumerate(rows):
            sq = float(np.sum((e["value"][r] - e["reference"][r]) ** 2))
            assert sq <= 4.0 * plan["cutoff"][k] ** 2 * (1 + 1e-9), (b, k, sq)
        if kind == "zero":
            assert (e["rewards"] == 1.0).all() and np.array_equal(e["value"], e["reference"])
        if kind == "cutoff":
            assert np.abs(e["rewards"] - ref["CUTOFF_ESP"]).max() < 1e-12
        if kind == "below":
            assert e["value"][0] < 0.0
        lanes.append(lane)
    case = {k: np.stack([lane[k] for lane in lanes], -1) for k in INPUTS}
    case.update({f"expected.{k}": np.stack([lane["expected"][k] for lane in lanes], -1) for k in OUTPUTS})
    case.update({f"plan.{k}": np.asarray(v) for k, v in plan.items()})
    return case


CASES = (
    # label, contacts, motors, frames of the true side, frames of the reference side
    ("quadruped", 4, 12, 6, 5),
    ("one", 1, 1, 2, 3),
)


def main(out_path: str, verbose: bool = True) -> None:
    ref = load_reference_functions()
    rg = np.random.default_rng(SEED)
    out: dict = {}
    for label, *args in CASES:
        for k, v in make_case(ref, rg, *args).items():
            out[f"{label}.{k}"] = v
    out["cases"] = np.array([c[0] for c in CASES])
    out["designed_lanes"] = np.array(DESIGNED)
    out["cutoff_esp"] = np.array(ref["CUTOFF_ESP"])
    out["tier"] = np.array("A: the reference's compute_height, quat_apply and radial_basis_function on the arrays they are written "
                           "for; the reads of the pose columns, the velocity mask and the subtraction are restated")
    np.savez_compressed(out_path, **out)
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if not os.path.isdir(COMMON):
        sys.exit(f"{COMMON} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            fresh = os.path.join(tmp, "ref_tracking_rewards.npz")
            main(fresh, verbose=False)
            same = open(fresh, "rb").read() == open(OUT, "rb").read()
        print("tests/golden/ref_tracking_rewards.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
