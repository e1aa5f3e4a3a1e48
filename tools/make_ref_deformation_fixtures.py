"""Reference-pinned fixtures of the DeformationEstimator block: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_block_fixtures.py: the arithmetic of the block is plain Python under
`numba.jit`; this script parses the reference files where they lie, takes the function definitions named in SOURCES
(decorators included) and executes them with `numba.jit` stubbed to the identity.  Nothing of the reference is copied
into the repository: only authored descriptions, seeded inputs and the outputs the reference's code produced for them,
written to tests/golden/ref_deformation.npz.

Run where the reference tree is available:   python tools/make_ref_deformation_fixtures.py [output.npz]

Two kinds of cases:

* ESTIMATOR cases (tier A: the reference's functions on the data they are written for).  An authored kinematic
  description -- frames as lists of (constant rotation, joint rotation about an axis by an encoder angle) segments, in
  the layout of `jm_deform_desc` -- and seeded encoder angles; this script computes the frame rotations from them in
  numpy and hands them, lane by lane, to the reference's `flexibility_estimator` and `quat_to_rpy`.
  The branch tests of `matrices_to_quat` and `swing_from_vector` and the branch cuts of the Euler angles are
  discontinuous: a lane within 1e-3 of one of them (for the 1e-5-wide tests of `swing_from_vector`: within a factor 2 of
  the threshold), or with a pitch within 1e-2 of +-pi/2, is rejected and drawn again, so that every stored lane counts.
  In the singular branch of `swing_from_vector` the reference reads a flag (`esp_ratio`) that it only assigns when
  exactly one of |v_x|, |v_y| is below 1e-5; no lane is drawn where neither is (plain Python raises there).
* CHAIN cases (tier B: reference text on a stand-in).  `get_flexibility_imu_frame_chains` on a ten-line stand-in for
  the pinocchio model (`parents`, `frames[i].parent`, `get_frame_indices`, `jiminy.get_joint_type`): the chains, or the
  exception class and message.
"""
from __future__ import annotations

import ast
import json
import os
import sys
import types
import typing

import numpy as np

REF = os.environ.get("JIMINY_REFERENCE", "/root/reference")
COMMON = os.path.join(REF, "python/gym_jiminy/common/gym_jiminy/common")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_deformation.npz")

SOURCES = {
    "utils/math.py": ("compute_tilt_from_quat", "swing_from_vector", "matrices_to_quat", "quat_multiply", "quat_to_rpy"),
    "blocks/deformation_estimator.py": ("_compute_orientation_error", "_compute_deformation_from_deviation",
                                        "flexibility_estimator", "get_flexibility_imu_frame_chains"),
}
B = 64          # lanes per estimator case
SEED = 20261016


class _JointModelType:
    FREE, ROTARY = "free", "rotary"


class _Frame:
    def __init__(self, name: str, parent: int) -> None:
        self.name, self.parent = name, parent


class StandInModel:
    """What `get_flexibility_imu_frame_chains` reads of a pinocchio model."""

    def __init__(self, tree: dict) -> None:
        self.names = [j[0] for j in tree["joints"]]
        self.parents = [j[1] for j in tree["joints"]]
        self.root_free = bool(tree["root_free"])
        self.frames = [_Frame(n, i) for i, n in enumerate(self.names)]
        self.frames += [_Frame(n, j) for n, j in tree["imu"].items() if n not in self.names]


def load_reference_functions() -> dict:
    """Namespace holding the reference's functions, compiled from the reference's files where they lie."""
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    jiminy = types.SimpleNamespace(JointModelType=_JointModelType,
                                   get_joint_type=lambda model, index: (_JointModelType.FREE if model.root_free and index == 1
                                                                        else _JointModelType.ROTARY))

    def get_frame_indices(model, names):
        return [[f.name for f in model.frames].index(n) for n in names]

    ns: dict = {"np": np, "nb": nb, "jiminy": jiminy, "get_frame_indices": get_frame_indices,
                "pin": types.SimpleNamespace(Model=object), "ArrayOrScalar": typing.Any}
    ns.update({k: getattr(typing, k) for k in ("Optional", "Tuple", "Union", "List", "Sequence", "Dict", "Literal", "overload",
                                               "no_type_check")})
    for rel, names in SOURCES.items():
        path = os.path.join(COMMON, rel)
        with open(path) as f:
            tree = ast.parse(f.read(), filename=path)
        for node in tree.body:      # module-level constants (TWIST_SWING_SINGULAR_THR)
            if isinstance(node, ast.Assign) and all(isinstance(t, ast.Name) for t in node.targets) \
                    and isinstance(node.value, ast.Constant):
                exec(compile(ast.Module([node], []), path, "exec"), ns)
        found = set()
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and node.name in names:
                exec(compile(ast.Module([node], []), path, "exec"), ns)
                found.add(node.name)
        missing = set(names) - found
        if missing:
            raise RuntimeError(f"{rel}: functions {sorted(missing)} not found")
    return ns


# ---------------------------------------------------------------------------------------------- small rotation helpers
def rot_rpy(r: float, p: float, y: float) -> np.ndarray:
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]]) @ \
        np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])


def rot_axis_angle(axis: np.ndarray, angle: float) -> np.ndarray:
    a = np.asarray(axis, dtype=np.float64)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.cos(angle) * np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * np.outer(a, a)


def quat_axis_angle(axis: np.ndarray, angle: float) -> np.ndarray:
    return np.array([*(np.asarray(axis) * np.sin(angle / 2)), np.cos(angle / 2)])


def qmul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def quat_of(R: np.ndarray) -> np.ndarray:
    """A unit quaternion of the rotation R (largest-component method; its sign is of no consequence here)."""
    c = np.array([1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2],
                  1 + R[0, 0] + R[1, 1] + R[2, 2]])
    k = int(np.argmax(c))
    if k == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], c[3]])
    elif k == 0:
        q = np.array([c[0], R[1, 0] + R[0, 1], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]])
    elif k == 1:
        q = np.array([R[1, 0] + R[0, 1], c[1], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]])
    else:
        q = np.array([R[0, 2] + R[2, 0], R[2, 1] + R[1, 2], c[2], R[1, 0] - R[0, 1]])
    return q / np.linalg.norm(q)


def random_unit(rg: np.random.Generator) -> np.ndarray:
    v = rg.normal(size=3)
    return v / np.linalg.norm(v)


# ------------------------------------------------------------------------------------------- authored descriptions
SEG_NONE, SEG_X, SEG_Y, SEG_Z, SEG_AXIS = 0, 1, 2, 3, 4


class Description:
    """Frames as segment lists + chains, in the layout of `jm_deform_desc`."""

    def __init__(self, n_imu: int, n_enc: int) -> None:
        self.n_imu, self.n_enc = n_imu, n_enc
        self.frame_seg_start = [0]
        self.seg_kind, self.seg_enc, self.seg_rot, self.seg_axis, self.seg_ratio = [], [], [], [], []
        self.chain_nflex, self.chain_orphan, self.chain_imu, self.chain_imu_frame = [], [], [], []
        self.flex_frame, self.flex_flipped = [], []

    def frame(self, *segments) -> int:
        """segments: (rpy of the constant rotation, kind, encoder, ratio[, axis])"""
        for seg in segments:
            rpy, kind, enc, ratio = seg[:4]
            self.seg_rot.append(rot_rpy(*rpy))
            self.seg_kind.append(kind)
            self.seg_enc.append(enc)
            self.seg_ratio.append(ratio)
            self.seg_axis.append(np.asarray(seg[4], dtype=np.float64) if len(seg) > 4 else np.zeros(3))
        self.frame_seg_start.append(len(self.seg_kind))
        return len(self.frame_seg_start) - 2

    def chain(self, imus, flexs, child_orphan: bool) -> None:
        """imus: [(imu column, frame)], flexs: [(frame, flipped)]"""
        assert len(imus) == len(flexs) + 1 - int(child_orphan)
        self.chain_nflex.append(len(flexs))
        self.chain_orphan.append([0, int(child_orphan)])
        for col, fr in imus:
            self.chain_imu.append(col)
            self.chain_imu_frame.append(fr)
        for fr, flipped in flexs:
            self.flex_frame.append(fr)
            self.flex_flipped.append(int(flipped))

    def arrays(self) -> dict:
        i32 = lambda x: np.asarray(x, dtype=np.int32)       # noqa: E731
        return dict(n_imu=np.int32(self.n_imu), n_enc=np.int32(self.n_enc), chain_nflex=i32(self.chain_nflex),
                    chain_orphan=i32(self.chain_orphan), chain_imu=i32(self.chain_imu), chain_imu_frame=i32(self.chain_imu_frame),
                    flex_frame=i32(self.flex_frame), flex_flipped=i32(self.flex_flipped), frame_seg_start=i32(self.frame_seg_start),
                    seg_kind=i32(self.seg_kind), seg_enc=i32(self.seg_enc), seg_rot=np.array(self.seg_rot),
                    seg_axis=np.array(self.seg_axis), seg_ratio=np.asarray(self.seg_ratio, dtype=np.float64))

    def encoder_ratio(self, enc: int) -> float:
        return next((r for r, e, k in zip(self.seg_ratio, self.seg_enc, self.seg_kind) if k != SEG_NONE and e == enc), 1.0)

    def frame_rotation(self, f: int, angles: np.ndarray) -> np.ndarray:
        """Rotation of frame f for the encoder positions `angles` [n_enc] (numpy, one lane)."""
        R = np.eye(3)
        for s in range(self.frame_seg_start[f], self.frame_seg_start[f + 1]):
            R = R @ self.seg_rot[s]
            k = self.seg_kind[s]
            if k != SEG_NONE:
                axis = self.seg_axis[s] if k == SEG_AXIS else np.eye(3)[k - 1]
                R = R @ rot_axis_angle(axis, self.seg_ratio[s] * angles[self.seg_enc[s]])
        return R


def description_arm4() -> Description:
    """Fixed base, one chain of 4 flexibility points, leaf first, the base end without IMU: `is_chain_orphan` (False, True)."""
    d = Description(n_imu=5, n_enc=3)
    j1 = ((0.2, 0.1, -0.3), SEG_Y, 0, 0.1)                       # motor-side encoder, reduction 10
    j2 = ((0.0, 0.0, 0.0), SEG_X, 2, 1.0)
    imu = [d.frame(j1, j2, ((0.1, 1.2, -2.5), SEG_NONE, -1, 0.0)), d.frame(j1, j2, ((2.8, 0.2, 1.1), SEG_NONE, -1, 0.0)),
           d.frame(j1, ((-0.3, -0.6, 0.4), SEG_NONE, -1, 0.0)), d.frame(j1, ((0.5, 0.1, -0.2), SEG_NONE, -1, 0.0))]
    fl = [d.frame(j1, j2), d.frame(j1), d.frame(j1), d.frame(j1)]
    d.chain([(2, imu[0]), (0, imu[1]), (4, imu[2]), (1, imu[3])], [(f, True) for f in fl], child_orphan=True)
    return d


def description_star() -> Description:
    """Free-flyer star: one chain through the root body, two flexibility points, flipped flags mixed, (False, False).
    Frames turned far from the identity: with the joint angles they reach every branch of `matrices_to_quat`."""
    d = Description(n_imu=3, n_enc=2)
    ja = ((1.9, -0.7, 2.4), SEG_Z, 0, 1.0)
    jb = ((-2.6, 0.9, 0.8), SEG_AXIS, 1, 0.5, np.array([0.6, 0.0, 0.8]))
    imu = [d.frame(ja, ((0.3, 2.0, -1.0), SEG_NONE, -1, 0.0)), d.frame(((3.0, 0.4, -2.0), SEG_NONE, -1, 0.0)),
           d.frame(jb, ((-1.5, -1.0, 2.9), SEG_NONE, -1, 0.0))]
    d.chain([(1, imu[0]), (2, imu[1]), (0, imu[2])], [(d.frame(((2.2, 0.3, 1.0), SEG_NONE, -1, 0.0)), True),
                                                      (d.frame(((-0.4, -2.7, 0.6), SEG_NONE, -1, 0.0)), False)], child_orphan=False)
    return d


def description_two_chains() -> Description:
    """Two chains in one robot: 1 flexibility point with both IMUs, and 2 points whose last one is an orphan; one IMU
    column is not used at all."""
    d = Description(n_imu=5, n_enc=2)
    ja = ((0.4, -1.3, 2.0), SEG_X, 1, 1.0)
    jb = ((-2.0, 0.5, -0.9), SEG_Y, 0, 0.02)
    i0, i1 = d.frame(ja, ((1.0, 0.2, 0.3), SEG_NONE, -1, 0.0)), d.frame(((0.0, 0.0, 0.0), SEG_NONE, -1, 0.0))
    d.chain([(4, i0), (1, i1)], [(d.frame(ja), False)], child_orphan=False)
    i2, i3 = d.frame(jb, ja, ((-0.8, 0.9, 2.2), SEG_NONE, -1, 0.0)), d.frame(jb, ((2.5, -0.3, -1.7), SEG_NONE, -1, 0.0))
    d.chain([(0, i2), (3, i3)], [(d.frame(jb, ja), True), (d.frame(jb), False)], child_orphan=True)
    return d


# ------------------------------------------------------------------------------------------------- estimator cases
M2Q_MARGIN, THR, RPY_MARGIN, PITCH_MARGIN = 1e-3, 1e-5, 1e-3, 1e-2


def m2q_branch(R: np.ndarray):
    """(branch index of `matrices_to_quat`, distance to its nearest branch test)."""
    if R[2, 2] < 0:
        return (0 if R[0, 0] > R[1, 1] else 1), min(abs(R[2, 2]), abs(R[0, 0] - R[1, 1]))
    return (2 if R[0, 0] < -R[1, 1] else 3), min(abs(R[2, 2]), abs(R[0, 0] + R[1, 1]))


def swing_branch(v: np.ndarray):
    """(branch name of `swing_from_vector` for the tilt v, whether v keeps the margins); None: undefined in the reference."""
    vx, vy, vz = v
    if vz >= -1.0 + THR:
        return "regular", vz >= -1.0 + 2 * THR
    ok = vz <= -1.0 + THR / 2
    eps = []
    for c in (vx, vy):
        eps.append(abs(c) < THR)
        ok &= abs(c) <= THR / 2 or abs(c) >= 2 * THR
    if eps[0] and eps[1]:
        return "xy", ok
    if not eps[0] and not eps[1]:
        return None, False
    ratio = vx / vy if eps[0] else vy / vx
    t = np.sqrt(THR)
    ok &= abs(ratio) <= t / 2 or abs(ratio) >= 2 * t
    if abs(ratio) < t:
        return ("ratio_x" if eps[0] else "ratio_y"), ok
    return ("general_x" if eps[0] else "general_y"), ok


def singular_tilt(rg: np.random.Generator, kind: str) -> np.ndarray:
    """A unit tilt in the singular region of `swing_from_vector`, inside branch `kind`, away from its tests."""
    sg = lambda: rg.choice([-1.0, 1.0])      # noqa: E731
    if kind == "xy":
        a, b = sg() * rg.uniform(3e-6, 5e-6), sg() * rg.uniform(3e-6, 5e-6)
    elif kind in ("ratio_x", "ratio_y"):
        a, b = sg() * rg.uniform(1e-7, 1.5e-6), sg() * rg.uniform(1e-3, 3e-3)
    else:
        b = sg() * rg.uniform(4e-4, 7e-4)
        a = sg() * rg.uniform(6.4e-3, min(1.2e-2, 5e-6 / abs(b))) * abs(b)
    vx, vy = (a, b) if kind in ("xy", "ratio_x", "general_x") else (b, a)
    return np.array([vx, vy, -np.sqrt(1.0 - vx * vx - vy * vy)])


def quat_with_tilt(rg: np.random.Generator, u: np.ndarray) -> np.ndarray:
    """A unit quaternion q with R(q)^T e_z = u: the swing taking u to e_z, then any yaw."""
    axis = np.cross(u, [0.0, 0.0, 1.0])
    s = np.linalg.norm(axis)
    # (u along the vertical itself: any horizontal axis does)
    swing = quat_axis_angle(axis / s if s > 1e-12 else np.array([1.0, 0.0, 0.0]), np.arctan2(s, u[2]))
    return qmul(quat_axis_angle(np.array([0.0, 0.0, 1.0]), rg.uniform(-np.pi, np.pi)), swing)


def run_reference(ref: dict, d: Description, c: int, imu_quat: np.ndarray, kin_imu, kin_flex, ignore_twist: bool) -> np.ndarray:
    """`flexibility_estimator` for chain c of one lane; returns the deformation quaternions [4][K]."""
    K = d.chain_nflex[c]
    M = K + 1 - d.chain_orphan[c][1]
    i0 = sum(d.chain_nflex[k] + 1 - d.chain_orphan[k][1] for k in range(c))
    indices = tuple(int(x) for x in d.chain_imu[i0:i0 + M])
    f0 = sum(d.chain_nflex[:c])
    out = np.full((4, K), np.nan)
    ref["flexibility_estimator"](
        np.ascontiguousarray(imu_quat), indices, np.empty((4, M)), tuple(kin_imu), np.empty((4, M)), tuple(kin_flex),
        np.empty((4, K)), np.array(d.flex_flipped[f0:f0 + K], dtype=bool), (False, bool(d.chain_orphan[c][1])),
        np.empty((4, M)), np.empty((4, K)), np.empty((4, K)), out, ignore_twist)
    return out


def estimator_case(ref: dict, rg: np.random.Generator, d: Description, ignore_twist: bool, singular: str = "") -> dict:
    """B accepted lanes.  `singular`: name of the `swing_from_vector` branch ONE IMU of every second lane is put in (its
    position in the chain rotates with the lane); the other lanes, and the other IMUs of these lanes, are regular."""
    n_chain, nflex = len(d.chain_nflex), sum(d.chain_nflex)
    enc = np.zeros((d.n_enc, 2, B))
    imu = np.zeros((4, d.n_imu, B))
    quat, rpy = np.zeros((4, nflex, B)), np.zeros((3, nflex, B))
    m2q_hits, swing_hits, rejected, lane = np.zeros(4, dtype=np.int64), {}, 0, 0
    while lane < B:
        # joint angles within +-1.2 rad; the encoder reads them on its own side (motor side: angle / ratio)
        angles = rg.uniform(-1.2, 1.2, size=d.n_enc) / np.array([d.encoder_ratio(i) for i in range(d.n_enc)])
        q_obs = rg.normal(size=(4, d.n_imu))
        q_obs /= np.linalg.norm(q_obs, axis=0, keepdims=True)       # (columns no chain reads stay random)
        ok, out_q, branches, swings = True, [], [], []
        i0 = 0
        for c in range(n_chain):
            K = d.chain_nflex[c]
            M = K + 1 - d.chain_orphan[c][1]
            f0 = sum(d.chain_nflex[:c])
            kin_imu = [d.frame_rotation(d.chain_imu_frame[i0 + i], angles) for i in range(M)]
            kin_flex = [d.frame_rotation(d.flex_frame[f0 + k], angles) for k in range(K)]
            which = (lane // 2) % M if (singular and lane % 2 == 0) else -1
            for i in range(M):
                col = d.chain_imu[i0 + i]
                if i == which:
                    q_obs[:, col] = quat_with_tilt(rg, kin_imu[i].T @ singular_tilt(rg, singular))
                else:
                    # the kinematic orientation turned by up to 0.6 rad about a random axis
                    q_obs[:, col] = qmul(quat_axis_angle(random_unit(rg), rg.uniform(-0.6, 0.6)), quat_of(kin_imu[i]))
            for R in kin_flex + ([] if ignore_twist else kin_imu):
                br, dist = m2q_branch(R)
                branches.append(br)
                ok &= dist >= M2Q_MARGIN
            if ignore_twist:
                tilt = np.stack(ref["compute_tilt_from_quat"](np.ascontiguousarray(q_obs[:, d.chain_imu[i0:i0 + M]])), 1)
                for i in range(M):
                    name, keeps = swing_branch(kin_imu[i] @ tilt[i])
                    ok &= bool(keeps) and (name == (singular if i == which else "regular"))
                    swings.append(name)
            if ok:
                out_q.append(run_reference(ref, d, c, q_obs, kin_imu, kin_flex, ignore_twist))
            i0 += M
        if ok:
            q = np.concatenate(out_q, axis=1)
            e = np.empty((3, nflex))
            ref["quat_to_rpy"](q, e)
            ok = bool(np.isfinite(q).all() and np.isfinite(e).all() and (np.abs(e[1]) <= np.pi / 2 - PITCH_MARGIN).all()
                      and (np.abs(e[[0, 2]]) <= np.pi - RPY_MARGIN).all())
        if not ok:
            rejected += 1
            if rejected > 200 * B:
                raise RuntimeError("too many rejected lanes: the description cannot keep the margins")
            continue
        enc[:, 0, lane], enc[:, 1, lane] = angles, rg.normal(size=d.n_enc)
        imu[:, :, lane], quat[:, :, lane], rpy[:, :, lane] = q_obs, q, e
        for br in branches:
            m2q_hits[br] += 1
        for s in swings:
            swing_hits[s] = swing_hits.get(s, 0) + 1
        lane += 1
    case = d.arrays()
    case.update(ignore_twist=np.int32(ignore_twist), enc=enc, imu_quat=imu, quat=quat, rpy=rpy, m2q_hits=m2q_hits,
                singular=np.array(singular), swing_hits=np.array(json.dumps(swing_hits, sort_keys=True)))
    return case, rejected


# ----------------------------------------------------------------------------------------------------- chain cases
def _tree(joints, root_free, flex, imu) -> dict:
    names = [j[0] for j in joints]
    return {"joints": [[n, (names.index(p) if p else 0)] for n, p in joints], "root_free": root_free, "flex": list(flex),
            "imu": {k: names.index(v) for k, v in imu.items()}}


CHAIN_TREES = {
    # the three of the issue text
    "fixed_chain": _tree([("universe", None), ("j1", "universe"), ("fa", "j1"), ("j2", "fa"), ("fb", "j2"), ("j3", "fb")],
                         False, ["fa", "fb"], {"j2": "j2", "j3": "j3"}),
    "ff_chain": _tree([("universe", None), ("root", "universe"), ("fa", "root"), ("j2", "fa"), ("fb", "j2"), ("j3", "fb")],
                      True, ["fa", "fb"], {"root": "root", "j2": "j2", "j3": "j3"}),
    "ff_star": _tree([("universe", None), ("root", "universe"), ("fa", "root"), ("la", "fa"), ("fb", "root"), ("lb", "fb")],
                     True, ["fa", "fb"], {"root": "root", "la": "la", "lb": "lb"}),
    # the arm of the reference's own unit test: every IMU sits on the body of a flexibility joint
    "arm_imu_on_flex": _tree([("universe", None), ("base_to_link1", "universe"), ("f12", "base_to_link1"), ("f23", "f12"),
                              ("f34", "f23"), ("f45", "f34")], False, ["f12", "f23", "f34", "f45"],
                             {"f12": "f12", "f23": "f23", "f34": "f34", "f45": "f45"}),
    # tests/data/flex_arm.urdf as tests/robots_deformation.py compiles it (joint order of the compiled model)
    "flex_arm": _tree([("universe", None), ("shoulder", "universe"), ("f12", "shoulder"), ("f23", "f12"),
                       ("elbowFlexibility", "f23"), ("elbow", "elbowFlexibility"), ("f45", "elbow")], False,
                      ["f12", "f23", "elbowFlexibility", "f45"], {"imu2": "f12", "imu3": "f23", "imu4": "elbow", "imu5": "f45"}),
    "flex_arm_ff": _tree([("universe", None), ("root_joint", "universe"), ("shoulder", "root_joint"), ("f12", "shoulder"),
                          ("f23", "f12"), ("elbowFlexibility", "f23"), ("elbow", "elbowFlexibility"), ("f45", "elbow")], True,
                         ["f12", "f23", "elbowFlexibility", "f45"],
                         {"imu0": "root_joint", "imu2": "f12", "imu3": "f23", "imu4": "elbow", "imu5": "f45"}),
    # free-flyer without IMU on the root: the chain comes out with a missing IMU (the block then refuses it)
    "flex_arm_ff_no_root_imu": _tree([("universe", None), ("root_joint", "universe"), ("shoulder", "root_joint"), ("f12", "shoulder"),
                                      ("f23", "f12"), ("elbowFlexibility", "f23"), ("elbow", "elbowFlexibility"), ("f45", "elbow")],
                                     True, ["f12", "f23", "elbowFlexibility", "f45"],
                                     {"imu2": "f12", "imu3": "f23", "imu4": "elbow", "imu5": "f45"}),
    # a fixed-base tree with two flexible branches and a flexible trunk
    "fixed_two_branches": _tree([("universe", None), ("j1", "universe"), ("ft", "j1"), ("trunk", "ft"), ("fa", "trunk"),
                                 ("la", "fa"), ("fb", "trunk"), ("lb", "fb")], False, ["ft", "fa", "fb"],
                                {"trunk": "trunk", "la": "la", "lb": "lb"}),
    # errors
    "error_imu_on_fixed_root": _tree([("universe", None), ("j1", "universe"), ("fa", "j1"), ("j2", "fa")], False, ["fa"],
                                     {"j1": "j1", "j2": "j2"}),
    "error_leaf_without_imu": _tree([("universe", None), ("j1", "universe"), ("fa", "j1"), ("j2", "fa"), ("fb", "j2"),
                                     ("j3", "fb")], False, ["fa", "fb"], {"j2": "j2"}),
    "error_not_interleaved": _tree([("universe", None), ("j1", "universe"), ("fa", "j1"), ("fb", "fa"), ("j2", "fb")], False,
                                   ["fa", "fb"], {"j2": "j2"}),
}


def chain_case(ref: dict, tree: dict):
    try:
        chains = ref["get_flexibility_imu_frame_chains"](StandInModel(tree), list(tree["flex"]), list(tree["imu"]))
        return {"chains": [[list(f), list(i), [bool(x) for x in fl]] for f, i, fl in chains]}
    except Exception as e:      # noqa: BLE001  (the class and the message ARE the recorded result)
        return {"error": [type(e).__name__, str(e)]}


def main(out_path: str) -> None:
    ref = load_reference_functions()
    rg = np.random.default_rng(SEED)
    out: dict = {}
    cases = [("arm4", description_arm4, False, ""), ("arm4", description_arm4, True, ""),
             ("star", description_star, False, ""), ("star", description_star, True, ""),
             ("two_chains", description_two_chains, False, ""), ("two_chains", description_two_chains, True, "")]
    cases += [("arm4", description_arm4, True, s) for s in ("xy", "ratio_x", "ratio_y", "general_x", "general_y")]
    cases += [("two_chains", description_two_chains, True, "xy")]
    names = []
    for name, make, ignore_twist, singular in cases:
        label = f"{name}_{'swing' if ignore_twist else 'twist'}" + (f"_{singular}" if singular else "")
        case, rejected = estimator_case(ref, rg, make(), ignore_twist, singular)
        for k, v in case.items():
            out[f"est.{label}.{k}"] = v
        names.append(label)
        print(f"{label}: {rejected} lanes rejected, matrices_to_quat branches {case['m2q_hits'].tolist()}, "
              f"swing_from_vector {case['swing_hits']}")
    m2q_total = sum(out[f"est.{n}.m2q_hits"] for n in names)
    if (m2q_total == 0).any():
        raise RuntimeError(f"a branch of matrices_to_quat is not covered: {m2q_total}")
    out["est_cases"] = np.array(names)
    out["chain_cases"] = np.array(json.dumps({k: {"tier": "B", "tree": t, "result": chain_case(ref, t)} for k, t in CHAIN_TREES.items()},
                                             sort_keys=True))
    np.savez_compressed(out_path, **out)
    print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")
    for k, v in json.loads(str(out["chain_cases"])).items():
        print(f"  {k}: {v['result']}")


if __name__ == "__main__":
    if not os.path.isdir(COMMON):
        sys.exit(f"{COMMON} not found: run this where the reference tree is available")
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
