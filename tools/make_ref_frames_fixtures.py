"""Reference-pinned fixtures of the SE3 step average of the frame kinematics block: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_attitude_fixtures.py: this script parses the reference files where they lie,
takes the function definitions named in SOURCES (decorators included) and executes them with `numba.jit` stubbed to the
identity.  Nothing of the reference is copied into the repository: only authored descriptions, seeded inputs and the
outputs the reference's code produced for them, written to tests/golden/ref_frames.npz.

Run where the reference tree is available:   python tools/make_ref_frames_fixtures.py [output.npz]
                                             python tools/make_ref_frames_fixtures.py --check     (regenerate and compare)

Tier A for the functions, a restated composition for the glue: every number comes out of the reference's functions (`log3`,
`exp3`, `log6`, `exp6`, `quat_multiply`, `quat_apply`, `xyzquat_difference`, `remove_yaw_from_quat`, `quat_to_rpy`,
`compute_height`) called on the arrays they are written for, one lane at a time.  What this script RESTATES, and labels as
such below, is the glue around them: `integrate(p, w)` -- the pose `p` composed with `exp6(w)`, position `x + R(q) t_e` by
`quat_apply`, quaternion `q * q_e` by `quat_multiply`, where the reference calls `pin.liegroups.SE3().integrate` -- and the
ORDER in which the `refresh` bodies of the quantity classes call them (quantities/generic.py:1275-1286, 1357-1360, 1421-1426,
1522-1534; quantities/locomotion.py:281-288).

Every case holds 64 lanes and three consecutive steps: the previous pose carries over.  A lane is redrawn until, on every
step and frame, the pitch of the mean pose keeps 1e-2 from +-pi/2 and its roll and yaw keep 1e-3 from the +-pi cut; the
draw loop counts its redraws, so every stored lane counts.
"""
from __future__ import annotations

import ast
import os
import sys
import tempfile
import types
import typing

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_ref_deformation_fixtures as mdf     # noqa: E402  (authored helpers: rotations, margins)

REF = os.environ.get("JIMINY_REFERENCE", "/root/reference")
COMMON = os.path.join(REF, "python/gym_jiminy/common/gym_jiminy/common")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_frames.npz")

SOURCES = {
    "utils/math.py": ("log3", "exp3", "log6", "exp6", "quat_multiply", "quat_apply", "xyzquat_difference",
                      "remove_yaw_from_quat", "quat_to_rpy"),
    "quantities/locomotion.py": ("compute_height",),
}
B = 64
STEPS = 3
SEED = 20261019
STEP_DT = 0.04
LOCAL, LOCAL_WORLD_ALIGNED, ODOMETRY = 0, 1, 2
PITCH_MARGIN, CUT_MARGIN = 1e-2, 1e-3


def load_reference_functions() -> dict:
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    ns: dict = {"np": np, "nb": nb, "ArrayOrScalar": typing.Any}
    ns.update({k: getattr(typing, k) for k in ("Optional", "Tuple", "Union", "List", "Sequence", "Dict", "Literal", "overload",
                                               "no_type_check")})
    for rel, names in SOURCES.items():
        path = os.path.join(COMMON, rel)
        with open(path) as f:
            tree = ast.parse(f.read(), filename=path)
        found = set()
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and node.name in names:      # (typing overloads first, the definition last)
                exec(compile(ast.Module([node], []), path, "exec"), ns)
                found.add(node.name)
        if set(names) - found:
            raise RuntimeError(f"{rel}: functions {sorted(set(names) - found)} not found")
    return ns


# ------------------------------------------------------------------------------------------------------ restated glue
def integrate(ref: dict, xyzquat: np.ndarray, w: np.ndarray) -> np.ndarray:
    """RESTATED: `pin.liegroups.SE3().integrate(xyzquat, w)` as the pose composed with `exp6(w)`."""
    e = ref["exp6"](w)
    out = np.empty(7)
    out[:3] = xyzquat[:3] + ref["quat_apply"](xyzquat[3:], e[:3])
    out[3:] = ref["quat_multiply"](xyzquat[3:], e[3:])
    return out


def average_step(ref: dict, prev: np.ndarray, cur: np.ndarray, mode: int, inv_step_dt: float):
    """RESTATED ORDER of the quantity classes for one frame of one lane: `_DifferenceFrameXYZQuat` (generic.py:1284, with
    `xyzquat_difference` standing for the SE3 difference as utils/math.py documents), `AverageFrameXYZQuat` (:1359-1360),
    `AverageFrameRollPitch` (:1423), `FrameSpatialAverageVelocity` (:1524-1532), `BaseSpatialAverageVelocity`
    (locomotion.py:284-286)."""
    diff = ref["xyzquat_difference"](prev, cur)
    mean = integrate(ref, cur, - 0.5 * diff)
    quat_no_yaw = np.empty(4)
    ref["remove_yaw_from_quat"](mean[3:], quat_no_yaw)
    v_spatial = np.zeros(6)
    np.multiply(diff, inv_step_dt, v_spatial)
    v_lin_ang = v_spatial.reshape((2, 3)).T
    if mode == LOCAL_WORLD_ALIGNED:
        ref["quat_apply"](mean[3:], v_lin_ang, v_lin_ang)
    elif mode == ODOMETRY:
        out = np.zeros(6)
        ref["quat_apply"](quat_no_yaw, v_spatial.reshape((2, 3)).T, out.reshape((2, 3)).T)
        v_spatial = out
    rpy = np.empty(3)
    ref["quat_to_rpy"](mean[3:], rpy)
    return v_spatial, mean, quat_no_yaw, rpy


# ------------------------------------------------------------------------------------------------------------ cases
def random_pose(rg: np.random.Generator) -> np.ndarray:
    q = mdf.qmul(mdf.quat_axis_angle(np.array([0.0, 0.0, 1.0]), rg.uniform(-np.pi, np.pi)),
                 mdf.quat_axis_angle(mdf.random_unit(rg), rg.uniform(-1.0, 1.0)))
    return np.concatenate([rg.uniform(-2.0, 2.0, 3), q / np.linalg.norm(q)])


def next_pose(rg: np.random.Generator, pose: np.ndarray, angle, reach: float) -> np.ndarray:
    """The pose moved by a rotation of `angle` (log-uniform in the given range, random axis, applied on the right) and
    a world translation of at most `reach`."""
    theta = float(np.exp(rg.uniform(np.log(angle[0]), np.log(angle[1]))))
    q = mdf.qmul(pose[3:], mdf.quat_axis_angle(mdf.random_unit(rg), theta))
    return np.concatenate([pose[:3] + mdf.random_unit(rg) * rg.uniform(0.0, reach), q / np.linalg.norm(q)])


def make_case(ref: dict, rg: np.random.Generator, modes, angle, reach: float, rest_every: int = 0):
    K, inv_step_dt = len(modes), 1.0 / STEP_DT
    lanes, redraws = [], 0
    while len(lanes) < B:
        at_rest = bool(rest_every) and len(lanes) % rest_every == 0
        poses = np.empty((STEPS + 1, 7, K))
        out = dict(v_avg=np.empty((STEPS, 6, K)), pose_mean=np.empty((STEPS, 7, K)), quat_no_yaw=np.empty((STEPS, 4, K)))
        ok = True
        for k, mode in enumerate(modes):
            poses[0, :, k] = random_pose(rg)
            for t in range(STEPS):
                poses[t + 1, :, k] = poses[t, :, k] if at_rest else next_pose(rg, poses[t, :, k], angle, reach)
                v, mean, qny, rpy = average_step(ref, poses[t, :, k].copy(), poses[t + 1, :, k].copy(), mode, inv_step_dt)
                out["v_avg"][t, :, k], out["pose_mean"][t, :, k], out["quat_no_yaw"][t, :, k] = v, mean, qny
                ok &= bool(np.isfinite(np.concatenate([v, mean, qny, rpy])).all())
                ok &= bool(abs(rpy[1]) <= np.pi / 2 - PITCH_MARGIN and abs(rpy[0]) <= np.pi - CUT_MARGIN
                           and abs(rpy[2]) <= np.pi - CUT_MARGIN)
        if not ok:
            redraws += 1
            if redraws > 400 * B:
                raise RuntimeError("too many redrawn lanes")
            continue
        # `compute_height` of the first frame over the others (a frame alone: over itself), at every pose
        others = poses[:, :3, 1:] if K > 1 else poses[:, :3, :1]
        out["height"] = np.array([ref["compute_height"](poses[t, :3, 0], others[t]) for t in range(STEPS + 1)])
        out["pose"], out["rest"] = poses, np.bool_(at_rest)
        lanes.append(out)
    case = {k: np.stack([lane[k] for lane in lanes], -1) for k in lanes[0]}
    case.update(modes=np.asarray(modes, np.int32), inv_step_dt=np.float64(inv_step_dt))
    return case, redraws


CASES = (
    # label, modes, rotation between consecutive poses [rad], translation [m], every n-th lane at rest
    ("regular", (LOCAL, LOCAL_WORLD_ALIGNED, ODOMETRY), (1e-2, 1.0), 0.5, 0),
    ("rest", (LOCAL, LOCAL_WORLD_ALIGNED, ODOMETRY), (1e-2, 1.0), 0.5, 2),
    ("small_angle", (LOCAL, LOCAL_WORLD_ALIGNED, ODOMETRY), (1e-9, 1e-4), 0.5, 0),
    ("K1", (LOCAL_WORLD_ALIGNED,), (1e-2, 1.0), 0.5, 0),
)


def main(out_path: str, verbose: bool = True) -> None:
    ref = load_reference_functions()
    rg = np.random.default_rng(SEED)
    out: dict = {}
    for label, modes, angle, reach, rest_every in CASES:
        case, redraws = make_case(ref, rg, modes, angle, reach, rest_every)
        for k, v in case.items():
            out[f"{label}.{k}"] = v
        if verbose:
            print(f"{label}: {redraws} lanes redrawn")
    out["cases"] = np.array([c[0] for c in CASES])
    out["tier"] = np.array("A: the reference's functions on the arrays they are written for; `integrate` (the pose composed "
                           "with exp6) and the order of the quantity classes' refresh bodies are restated")
    np.savez_compressed(out_path, **out)
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if not os.path.isdir(COMMON):
        sys.exit(f"{COMMON} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            fresh = os.path.join(tmp, "ref_frames.npz")
            main(fresh, verbose=False)
            same = open(fresh, "rb").read() == open(OUT, "rb").read()
        print("tests/golden/ref_frames.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
