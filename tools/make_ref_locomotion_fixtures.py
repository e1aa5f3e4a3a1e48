"""Reference-pinned fixtures of the locomotion quantities block: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_frames_fixtures.py: this script parses the reference files where they lie, takes
the function definitions named in SOURCES (decorators included) and the constant `CUTOFF_ESP`, and executes them with
`numba.jit` stubbed to the identity.  Nothing of the reference is copied into the repository: only authored descriptions,
seeded inputs and the outputs the reference's code produced for them, written to tests/golden/ref_locomotion.npz.

Run where the reference tree is available:   python tools/make_ref_locomotion_fixtures.py [output.npz]
                                             python tools/make_ref_locomotion_fixtures.py --check     (regenerate and compare)

Tier A for the functions, a restated composition for the glue: `translate_position_odom`, `normalize_spatial_forces`,
`normalize_vertical_forces`, `min_depth`, `radial_basis_function`, `quat_to_yaw_cos_sin`, `quat_to_yaw` and `quat_apply` are the
reference's, called on the arrays they are written for, one lane at a time.  What this script RESTATES, and labels as such
below, are the `refresh` bodies of the quantity classes around them (they read `pinocchio_data`, which does not exist here):
`CenterOfMass`, `BaseOdometryPose` (on the root quaternion of `q`), `ZeroMomentPoint`, `CapturePoint`, `AverageBaseMomentum`,
`MultiContactNormalizedSpatialForce`, `MultiFootNormalizedForceVertical`, `_MultiContactMinGroundDistance`, and the data the
engine would have left: the mass of the robot as the sum of its bodies' in joint order, `vcom = hg_linear / mass`
(core/src/engine/engine.cc:896) and zero multipliers for a disabled contact constraint.

Every case holds 64 lanes.  The draw keeps `f_z / weight` in [0.2, 3], `|com_xy| <= 2`, `com_z` in [0.2, 1.5] and the argument
of both radial basis functions `err^2 / cutoff^2 <= 4`; in `free_fall` every second lane has `dhg_linear_z = -weight` exactly
(the masses and the gravity of that case are short binary fractions, so that the weight is the same number in float32).
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
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_locomotion.npz")

SOURCES = {
    "utils/math.py": ("quat_to_yaw_cos_sin", "quat_to_yaw", "quat_apply"),
    "quantities/locomotion.py": ("translate_position_odom", "normalize_spatial_forces", "normalize_vertical_forces"),
    "compositions/locomotion.py": ("min_depth",),
    "compositions/mixin.py": ("CUTOFF_ESP", "radial_basis_function"),
}
B = 64
SEED = 20261019
LOCAL, LOCAL_WORLD_ALIGNED = 0, 1
INPUTS = ("centroidal", "q_root", "model_lane", "con_lambda", "con_flags", "v_avg", "quat_no_yaw", "pose")
OUTPUTS = ("com", "vcom", "odom_pose", "zmp", "dcm", "h_angular", "contact_force_rel", "foot_force_vertical", "scalars")


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
def robot_mass(masses: np.ndarray) -> float:
    """RESTATED: `pinocchio_data.mass[0]` as the sum of the bodies' masses in joint order (joint 0 is the universe)."""
    total = 0.0
    for m in masses[1:]:
        total += float(m)
    return total


def lane_quantities(ref: dict, plan: dict, lane: dict) -> dict:
    """RESTATED `refresh` bodies of the quantity classes for one lane, around the reference's own functions:
    `CenterOfMass` (quantities/locomotion.py:878-887), `BaseOdometryPose` (:211-219), `ZeroMomentPoint` (:996-1017),
    `CapturePoint` (:1114-1124), `AverageBaseMomentum` (:404-412), `MultiContactNormalizedSpatialForce` (:1260-1268),
    `MultiFootNormalizedForceVertical` (:1468-1481), `_MultiContactMinGroundDistance` (compositions/locomotion.py:527-540) on flat
    ground, `MinimizeAngularMomentumReward` / `MinimizeFrictionReward` (:257-315)."""
    nc, n_feet = len(plan["contact_foot"]), int(plan["n_feet"])
    masses = lane["model_lane"][0::13] if "model_lane" in lane else plan["body_mass"]
    inertia6 = lane["model_lane"][13 + 4:13 + 10] if "model_lane" in lane else plan["root_inertia"]
    mass = robot_mass(masses)
    robot_weight = mass * abs(float(plan["gravity"]))
    c = lane["centroidal"]
    com, hg_linear, dhg_linear, dhg_angular = c[0:3].copy(), c[3:6], c[9:12], c[12:15]
    vcom = hg_linear / mass
    out = dict(com=com, vcom=vcom)

    odom_pose = np.zeros(3)
    odom_pose[:2] = lane["q_root"][:2]
    odom_pose[2] = float(ref["quat_to_yaw"](lane["q_root"][3:7].copy()))
    out["odom_pose"] = odom_pose

    zmp = np.zeros(2)
    f_z = dhg_linear[2] + robot_weight
    if abs(f_z) < np.finfo(np.float32).eps:
        zmp[:] = float("nan")
    else:
        zmp[:] = com[:2] * (robot_weight / f_z)
        zmp[0] -= (dhg_angular[1] + dhg_linear[0] * com[2]) / f_z
        zmp[1] += (dhg_angular[0] - dhg_linear[1] * com[2]) / f_z
        if plan["zmp_frame"] == LOCAL:
            ref["translate_position_odom"](zmp, odom_pose, zmp)
    out["zmp"] = zmp

    dcm = np.zeros(2)
    dcm[:] = com[:2] + vcom[:2] / float(plan["omega"])
    if plan["dcm_frame"] == LOCAL:
        ref["translate_position_odom"](dcm, odom_pose, dcm)
    out["dcm"] = dcm

    xx, xy, xz, yy, yz, zz = (float(v) for v in inertia6)
    inertia_local = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
    root = int(plan["root_column"])
    h_angular = np.zeros(3)
    np.matmul(inertia_local, lane["v_avg"][3:6, root].copy(), h_angular)
    ref["quat_apply"](lane["quat_no_yaw"][:, root].copy(), h_angular, h_angular)
    out["h_angular"] = h_angular

    # (a disabled constraint carries zero multipliers)
    lambda_c = (lane["con_lambda"].reshape(nc, 4) * ((lane["con_flags"] & 1) != 0)[:, None]).reshape(-1)
    force_rel = np.zeros((6, nc), order="C")
    ref["normalize_spatial_forces"](lambda_c, 0, 4 * nc, robot_weight, force_rel)
    out["contact_force_rel"] = force_rel
    feet = list(plan["contact_foot"])
    foot_slices = tuple((4 * feet.index(f), 4 * (len(feet) - feet[::-1].index(f))) for f in range(n_feet))
    vertical = tuple(np.asfortranarray(np.tile(np.array([[0.0], [0.0], [1.0]]), (1, (e - s) // 4))) for s, e in foot_slices)
    foot_force = np.zeros(n_feet)
    ref["normalize_vertical_forces"](lambda_c, foot_slices, vertical, robot_weight, foot_force)
    out["foot_force_vertical"] = foot_force

    positions = np.asfortranarray(lane["pose"][:3][:, [int(k) for k in plan["contact_column"]]])
    normals = np.asfortranarray(np.tile(np.array([[0.0], [0.0], [1.0]]), (1, nc)))
    out["scalars"] = np.array([
        np.max(force_rel[2]),
        ref["min_depth"](positions, np.zeros(nc), normals),
        ref["radial_basis_function"](h_angular, float(plan["momentum_cutoff"]), 2),
        ref["radial_basis_function"](force_rel[:2], float(plan["friction_cutoff"]), 2)])
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def quat_axis_angle(axis: np.ndarray, angle: float) -> np.ndarray:
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])


def quat_mul(l: np.ndarray, r: np.ndarray) -> np.ndarray:
    return np.concatenate([l[3] * r[:3] + r[3] * l[:3] + np.cross(l[:3], r[:3]), [l[3] * r[3] - l[:3] @ r[:3]]])


def random_quat(rg: np.random.Generator, yaw: bool) -> np.ndarray:
    axis = rg.normal(size=3)
    axis[2] = 0.0 if not yaw else axis[2]
    q = quat_axis_angle(axis / np.linalg.norm(axis), rg.uniform(-1.0, 1.0))
    if yaw:
        q = quat_mul(quat_axis_angle(np.array([0.0, 0.0, 1.0]), rg.uniform(-np.pi, np.pi)), q)
    return q / np.linalg.norm(q)


def make_case(ref: dict, rg: np.random.Generator, contact_foot, n_feet: int, zmp_frame: int, dcm_frame: int, disable: bool,
              free_fall: bool, per_lane_model: bool):
    nc, nj = len(contact_foot), 6
    K = nc + 2
    columns = rg.permutation(K)
    # (free fall: short binary fractions, the weight is exact in float32 as well)
    body_mass = np.concatenate([[0.0], rg.integers(2, 40, nj - 1) / 4.0])
    gravity = 9.8125 if free_fall else 9.81
    d, o = rg.uniform(0.5, 2.0, 3), rg.uniform(-0.1, 0.1, 3)
    plan = dict(body_mass=body_mass, root_inertia=np.array([d[0], o[0], o[1], d[1], o[2], d[2]]), gravity=gravity,
                omega=float(rg.uniform(2.0, 5.0)), contact_foot=np.asarray(contact_foot, np.int32),
                contact_column=columns[1:1 + nc].astype(np.int32), n_feet=n_feet, n_frames=K, root_column=int(columns[0]),
                zmp_frame=zmp_frame, dcm_frame=dcm_frame, momentum_cutoff=float(rg.uniform(1.0, 4.0)),
                friction_cutoff=float(rg.uniform(0.5, 1.0)))
    lanes, designed_nan = [], []
    for b in range(B):
        lane: dict = {}
        if per_lane_model:
            ml = rg.uniform(-0.2, 0.2, (nj, 13))
            ml[:, 0] = rg.uniform(0.5, 8.0, nj)
            ml[:, 4], ml[:, 7], ml[:, 9] = rg.uniform(0.5, 2.0, (3, nj))
            ml[0] = 0.0
            lane["model_lane"] = ml.reshape(-1)
        mass = robot_mass(lane["model_lane"][0::13] if per_lane_model else body_mass)
        weight = mass * gravity
        falling = free_fall and b % 2 == 1
        designed_nan.append(falling)
        c = np.empty(15)
        c[0:2], c[2] = rg.uniform(-2.0, 2.0, 2), rg.uniform(0.2, 1.5)
        c[3:6], c[6:9] = mass * rg.uniform(-1.0, 1.0, 3), rg.uniform(-5.0, 5.0, 3)
        c[9:11] = weight * rg.uniform(-0.5, 0.5, 2)
        c[11] = -weight if falling else weight * rg.uniform(0.2, 3.0) - weight
        c[12:15] = weight * rg.uniform(-0.3, 0.3, 3)
        lane["centroidal"] = c
        lane["q_root"] = np.concatenate([rg.uniform(-2.0, 2.0, 2), rg.uniform(0.3, 1.0, 1), random_quat(rg, True)])
        lam = np.empty((nc, 4))
        lam[:, :2] = weight * rg.uniform(-0.2, 0.2, (nc, 2))
        lam[:, 2] = weight * rg.uniform(0.0, 1.0, nc)
        lam[:, 3] = weight * rg.uniform(-0.05, 0.05, nc)
        lane["con_lambda"] = lam.reshape(-1)
        flags = np.ones(nc, np.int32) | (rg.integers(0, 2, nc).astype(np.int32) << 1)      # (bit 1 is not the enabled bit)
        if disable:
            flags &= ~(rg.uniform(size=nc) < 0.3).astype(np.int32)
        lane["con_flags"] = flags
        v_avg, qny, pose = rg.uniform(-2.0, 2.0, (6, K)), np.empty((4, K)), np.empty((7, K))
        for k in range(K):
            qny[:, k] = random_quat(rg, False)
            pose[:, k] = np.concatenate([rg.uniform(-2.0, 2.0, 2), rg.uniform(-0.01, 0.5, 1), random_quat(rg, True)])
        lane.update(v_avg=v_avg, quat_no_yaw=qny, pose=pose)
        # the angular momentum scaled into the range of the momentum reward: |h| / cutoff uniform in [0, 2]
        h = np.linalg.norm(lane_quantities(ref, plan, lane)["h_angular"])
        v_avg[3:6] *= rg.uniform(0.0, 2.0) * plan["momentum_cutoff"] / h
        lane["expected"] = lane_quantities(ref, plan, lane)
        e = lane["expected"]
        assert np.sum(e["h_angular"] ** 2) <= 4.0 * plan["momentum_cutoff"] ** 2 * (1 + 1e-12)
        assert np.sum(e["contact_force_rel"][:2] ** 2) <= 4.0 * plan["friction_cutoff"] ** 2
        assert np.isnan(e["zmp"]).all() == falling and np.isnan(e["zmp"]).any() == falling
        lanes.append(lane)
    case = {k: np.stack([lane[k] for lane in lanes], -1) for k in INPUTS if k in lanes[0]}
    case.update({f"expected.{k}": np.stack([lane["expected"][k] for lane in lanes], -1) for k in OUTPUTS})
    case.update({f"plan.{k}": np.asarray(v) for k, v in plan.items()})
    case["designed_nan"] = np.asarray(designed_nan)
    return case


CASES = (
    # label, foot of every contact, feet, ZMP frame, DCM frame, some contacts disabled, free fall on odd lanes, per-lane model
    ("regular", (0, 1, 2, 3), 4, LOCAL, LOCAL, False, False, False),
    ("grouped", (0, 0, 0, -1, 1, 1, 1, 1), 2, LOCAL_WORLD_ALIGNED, LOCAL, True, False, False),
    ("one", (0,), 1, LOCAL, LOCAL_WORLD_ALIGNED, False, False, False),
    ("free_fall", (0, 1, 2, 3), 4, LOCAL, LOCAL, False, True, False),
    ("per_lane_model", (0, 0, 1, 1), 2, LOCAL, LOCAL, False, False, True),
)


def main(out_path: str, verbose: bool = True) -> None:
    ref = load_reference_functions()
    rg = np.random.default_rng(SEED)
    out: dict = {}
    for label, *args in CASES:
        for k, v in make_case(ref, rg, *args).items():
            out[f"{label}.{k}"] = v
    out["cases"] = np.array([c[0] for c in CASES])
    out["tier"] = np.array("A: the reference's functions on the arrays they are written for; the refresh bodies of the quantity "
                           "classes, the mass of the robot, vcom and the zero multipliers of a disabled contact are restated")
    np.savez_compressed(out_path, **out)
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if not os.path.isdir(COMMON):
        sys.exit(f"{COMMON} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            fresh = os.path.join(tmp, "ref_locomotion.npz")
            main(fresh, verbose=False)
            same = open(fresh, "rb").read() == open(OUT, "rb").read()
        print("tests/golden/ref_locomotion.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
