"""Reference-pinned fixtures of the foot pose quantities block: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_locomotion_fixtures.py: this script parses the reference files where they lie, takes
the function definitions named in SOURCES (decorators included) and the constant `CUTOFF_ESP`, and executes them with
`numba.jit` stubbed to the identity.  Nothing of the reference is copied into the repository: only authored descriptions,
seeded inputs and the outputs the reference's code produced for them, written to tests/golden/ref_footposes.npz.

Run where the reference tree is available:   python tools/make_ref_footposes_fixtures.py [output.npz]
                                             python tools/make_ref_footposes_fixtures.py --check     (regenerate and compare)

Tier A for the functions, a restated composition for the glue: `position_average`, `quat_average_2d`,
`quat_interpolate_middle`, `quat_to_matrix`, `translate_positions`, `quat_multiply`, `quat_to_yaw`, `log3`, `quat_difference` and
`radial_basis_function` are the reference's, called on the arrays they are written for, one lane at a time.  What this script
RESTATES, and labels as such below, are the `refresh` bodies of the quantity classes around them (`MultiFrameMeanXYZQuat`,
`MultiFootMeanOdometryPose`, `MultiFootRelativeXYZQuat`) and the composition of `TrackingQuantityReward` (`operator.sub` resp.
`quat_difference` of the true and the reference value, then the radial basis function).  One foot: `quat_average_2d` assigns
the `(4, 1)` array of quaternions to its output, which plain numpy only accepts for an output of that shape: the view of the
mean quaternion is passed as `(4, 1)` there.

Every case holds 64 lanes, K = F + 3 frames with the foot columns permuted among the others.  The orientations of the feet of a
lane lie within `spread` rad of a common uniformly random one and every quaternion is negated with probability 1 / 2 (q and
-q are one orientation).  On every lane of the cases of three feet or more the two largest eigenvalues of sum q q^T are at
least 0.1 apart relative to the largest (asserted here; SEED is one for which the wide case holds it).  `two_feet`: lane 0 is
(0, 0, 0, 1) and (1, 0, 0, 0), a dot product of exactly 0; lane 1 has a negative dot product.  `tracking`: the reference lies
within the cutoffs (both arguments of the radial basis function <= 4); on lane 0 it is the reference code's own output (the
position error is exactly 0, the orientation error what `quat_multiply` leaves of conj(q) q, a few 1e-17, and both rewards
are 1); on lane 1 the reference quaternion of the first foot is negated, so that the residual quaternion has w < 0.
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
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_footposes.npz")

SOURCES = {
    "utils/math.py": ("quat_to_yaw_cos_sin", "quat_to_yaw", "quat_to_matrix", "quat_multiply", "log3", "quat_difference",
                      "quat_interpolate_middle"),
    "quantities/generic.py": ("position_average", "quat_average_2d"),
    "quantities/locomotion.py": ("translate_positions",),
    "compositions/mixin.py": ("CUTOFF_ESP", "radial_basis_function"),
}
B = 64
SEED = 20261019
MIN_GAP = 0.1
OUTPUTS = ("mean_pose", "mean_odom_pose", "relative_pose", "tracking_error", "scalars")


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
def lane_quantities(ref: dict, plan: dict, pose: np.ndarray, reference=None) -> dict:
    """RESTATED `refresh` bodies for one lane, around the reference's own functions: `MultiFrameMeanXYZQuat`
    (quantities/generic.py:1055-1062), `MultiFootMeanOdometryPose` (quantities/locomotion.py:549-557), `MultiFootRelativeXYZQuat`
    (:779-810), and `TrackingQuantityReward` (compositions/generic.py:113-122) with the operators of
    `TrackingFootPositionsReward` / `TrackingFootOrientationsReward` (compositions/locomotion.py:167-214)."""
    columns = [int(c) for c in plan["foot_column"]]
    n_feet = len(columns)
    xyzquats = np.ascontiguousarray(pose[:, columns])
    positions, quats = xyzquats[:3], xyzquats[-4:]

    xyzquat_mean = np.zeros(7)
    ref["position_average"](positions, xyzquat_mean[:3])
    quat_mean = xyzquat_mean[3:]
    ref["quat_average_2d"](quats, quat_mean.reshape(4, 1) if n_feet == 1 else quat_mean)

    odom_pose = np.zeros(3)
    odom_pose[:2] = xyzquat_mean[:2]
    ref["quat_to_yaw"](xyzquat_mean[-4:], odom_pose[-1:].reshape(()))

    rot_mean = np.zeros((3, 3))
    foot_poses_rel = np.zeros((7, n_feet - 1))
    ref["quat_to_matrix"](quat_mean, rot_mean)
    ref["translate_positions"](positions[:, :-1], xyzquat_mean[:3], rot_mean, foot_poses_rel[:3])
    ref["quat_multiply"](quat_mean[:, np.newaxis], quats[:, :-1], foot_poses_rel[-4:], is_left_conjugate=True)
    out = dict(mean_pose=xyzquat_mean, mean_odom_pose=odom_pose, relative_pose=foot_poses_rel)

    if reference is not None or n_feet == 1:
        reference = np.zeros((7, 0)) if reference is None else reference
        error_position = foot_poses_rel[:3] - reference[:3]
        error_orientation = ref["quat_difference"](foot_poses_rel[-4:], reference[-4:])
        out["tracking_error"] = np.concatenate([error_position, error_orientation])
        out["scalars"] = np.array([ref["radial_basis_function"](error_position, float(plan["position_cutoff"]), 2),
                                   ref["radial_basis_function"](error_orientation, float(plan["orientation_cutoff"]), 2)])
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def quat_axis_angle(axis: np.ndarray, angle: float) -> np.ndarray:
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])


def quat_mul(l: np.ndarray, r: np.ndarray) -> np.ndarray:
    return np.concatenate([l[3] * r[:3] + r[3] * l[:3] + np.cross(l[:3], r[:3]), [l[3] * r[3] - l[:3] @ r[:3]]])


def random_unit(rg: np.random.Generator, n: int) -> np.ndarray:
    v = rg.normal(size=n)
    return v / np.linalg.norm(v)


def near(rg: np.random.Generator, q: np.ndarray, spread: float) -> np.ndarray:
    """A unit quaternion within `spread` rad of `q`."""
    out = quat_mul(q, quat_axis_angle(random_unit(rg, 3), rg.uniform(0.0, spread)))
    return out / np.linalg.norm(out)


def relative_gap(quats: np.ndarray) -> float:
    lam = np.linalg.eigvalsh(quats @ quats.T)
    return float((lam[-1] - lam[-2]) / lam[-1])


def make_case(ref: dict, rg: np.random.Generator, label: str, n_feet: int, spread: float, tracking: bool):
    K = n_feet + 3
    columns = rg.permutation(K)[:n_feet]
    plan = dict(foot_column=columns.astype(np.int32), n_frames=K, position_cutoff=float(rg.uniform(0.2, 0.6)),
                orientation_cutoff=float(rg.uniform(0.3, 1.0)))
    poses, references, expected = [], [], []
    for b in range(B):
        pose = np.empty((7, K))
        pose[:3] = rg.uniform(-2.0, 2.0, (3, K))
        common = random_unit(rg, 4)
        for k in range(K):
            pose[3:, k] = near(rg, common, spread) * rg.choice([-1.0, 1.0])
        if label == "two_feet" and b == 0:
            pose[3:, columns[0]], pose[3:, columns[1]] = (0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 0.0)
        if label == "two_feet" and b == 1 and pose[3:, columns[0]] @ pose[3:, columns[1]] > 0.0:
            pose[3:, columns[1]] *= -1.0
        if n_feet >= 3:
            assert relative_gap(pose[3:, columns]) >= MIN_GAP, (label, b, relative_gap(pose[3:, columns]))
        reference = None
        if tracking:
            # the reference code's own output, moved by at most `cutoff` per term: both arguments of the kernel stay <= 4
            reference = lane_quantities(ref, plan, pose)["relative_pose"].copy()
            if b != 0:
                shift = rg.normal(size=(3, n_feet - 1))
                reference[:3] += shift * (rg.uniform(0.0, 1.9) * plan["position_cutoff"] / np.linalg.norm(shift))
                angles = rg.uniform(0.0, 1.0, n_feet - 1)
                angles *= rg.uniform(0.0, 1.9) * plan["orientation_cutoff"] / np.linalg.norm(angles)
                for f in range(n_feet - 1):
                    q = quat_mul(reference[3:, f], quat_axis_angle(random_unit(rg, 3), angles[f]))
                    reference[3:, f] = q / np.linalg.norm(q) * rg.choice([-1.0, 1.0])
            if b == 1:
                # w of the residual quaternion conj(relative) * reference is negative
                residual = ref["quat_multiply"](lane_quantities(ref, plan, pose)["relative_pose"][3:, 0], reference[3:, 0],
                                                is_left_conjugate=True)
                reference[3:, 0] *= -1.0 if residual[3] > 0.0 else 1.0
            references.append(reference)
        e = lane_quantities(ref, plan, pose, reference)
        if tracking:
            assert np.sum(e["tracking_error"][:3] ** 2) <= 4.0 * plan["position_cutoff"] ** 2
            assert np.sum(e["tracking_error"][3:] ** 2) <= 4.0 * plan["orientation_cutoff"] ** 2
        poses.append(pose)
        expected.append(e)
    case = {"pose": np.stack(poses, -1)}
    if tracking:
        case["reference_relative_pose"] = np.stack(references, -1)
    case.update({f"expected.{k}": np.stack([e[k] for e in expected], -1) for k in OUTPUTS if k in expected[0]})
    case.update({f"plan.{k}": np.asarray(v) for k, v in plan.items()})
    return case


CASES = (
    # label, feet, spread of the orientations [rad], with a reference
    ("one_foot", 1, 1.0, False),
    ("two_feet", 2, 1.0, False),
    ("three_feet", 3, 1.0, False),
    ("four_feet", 4, 1.0, False),
    ("four_feet_wide", 4, 2.0, False),
    ("tracking", 4, 1.0, True),
)


def main(out_path: str, verbose: bool = True) -> None:
    ref = load_reference_functions()
    rg = np.random.default_rng(SEED)
    out: dict = {}
    for label, *args in CASES:
        for k, v in make_case(ref, rg, label, *args).items():
            out[f"{label}.{k}"] = v
    out["cases"] = np.array([c[0] for c in CASES])
    out["tier"] = np.array("A: the reference's functions on the arrays they are written for; the refresh bodies of the quantity "
                           "classes and the composition of TrackingQuantityReward are restated")
    np.savez_compressed(out_path, **out)
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if not os.path.isdir(COMMON):
        sys.exit(f"{COMMON} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            fresh = os.path.join(tmp, "ref_footposes.npz")
            main(fresh, verbose=False)
            same = open(fresh, "rb").read() == open(OUT, "rb").read()
        print("tests/golden/ref_footposes.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
