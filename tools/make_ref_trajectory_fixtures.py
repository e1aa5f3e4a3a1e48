"""Reference-pinned fixtures of the reference trajectories block: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_actuation_fixtures.py: the reference files are parsed where they lie, the definitions
named in SOURCES (decorators included) are executed with `numba.jit` stubbed to the identity.  The loader below is that one
with two additions: a file outside gym_jiminy (jiminy_py/dynamics.py) and the names the definitions of that file need at the
time they are executed (`dataclass`, `fields`, `bisect_left`, the stand-ins of `pin` and `jiminy`).  Nothing of the reference
is copied into the repository: only authored datasets, seeded queries and the outputs the reference's code produced for them,
written to tests/golden/ref_trajectory.npz.

Run where the reference tree is available:   python tools/make_ref_trajectory_fixtures.py [output.npz]
                                             python tools/make_ref_trajectory_fixtures.py --check     (regenerate and compare)

Tier A, executed verbatim: `State`, `Trajectory` (`__init__`, `time_interval`, `get`), `TrajectoryTimeMode` and `TRAJ_INTERP_TOL`
of jiminy_py/dynamics.py; `log6`, `exp6`, `log3`, `exp3`, `quat_multiply`, `quat_apply` of gym_jiminy/common/utils/math.py;
`quat_to_yaw_cos_sin` / `quat_to_yaw` for the odometry pose.  Every expected state is what `Trajectory.get(t, mode)` returned
for one lane.

RESTATED, because pinocchio is not available where this runs, and labelled as such below: a stand-in for `pin` (an SE3
type with `*` and `inverse()`, `XYZQUATToSE3`, `SE3ToXYZQUAT`, `log6` / `exp6` on the reference's own functions, `interpolate`
joint by joint: a vector space `q0 + alpha (q1 - q0)`, the free-flyer `M0 exp6(alpha log6(M0^-1 M1))`, a spherical joint
`quat0 exp3(alpha log3(quat0^-1 quat1))`, an unbounded revolute joint the same on its angle); a robot stand-in with
`has_freeflyer` and the joint table; the offset formula of `DatasetTrajectoryQuantity._select`; `BaseOdometryPose.refresh`.

A case is a dataset and a few query events on 64 lanes; `expected.*` holds the tensors of the block after every event (a lane
an event leaves out keeps what it had, zeros before the first).  Sample times, lane times and offsets lie on a grid of 2^-12,
so `divmod`, the comparisons and the index are exact on both sides; so do the data but the quaternions and the cos / sin
pairs, which are normalised in float64.  Designed lanes of the case `anymal`, event 0 (asserted in `check_designed`): LANES
below.  Drawing conditions, asserted: outside the designed lanes t - t_left and t_right - t are at least 2^-12, but for a query
outside a trajectory of mode raise or clip, which is clipped onto an end sample; consecutive quaternions have a positive dot
product.
"""
from __future__ import annotations

import ast
import math
import os
import sys
import tempfile
import types
import typing
from bisect import bisect_left
from dataclasses import dataclass, fields

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from tests import trajectory_numpy as tn                  # noqa: E402  (names and layouts)

REF = os.environ.get("JIMINY_REFERENCE", "/root/reference")
COMMON = os.path.join(REF, "python/gym_jiminy/common/gym_jiminy/common")
DYNAMICS = os.path.join(REF, "python/jiminy_py/src/jiminy_py/dynamics.py")
OUT = os.path.join(HERE, "..", "tests", "golden", "ref_trajectory.npz")

SOURCES = {
    os.path.join(COMMON, "utils/math.py"): ("quat_to_yaw_cos_sin", "quat_to_yaw", "quat_multiply", "quat_apply", "log3", "exp3",
                                            "log6", "exp6"),
    DYNAMICS: ("TRAJ_INTERP_TOL", "State", "TrajectoryTimeMode", "Trajectory"),
}
B = 64
SEED = 20261021
GRID = 4096.0
RAISE, WRAP, CLIP = tn.RAISE, tn.WRAP, tn.CLIP
MODE_NAMES = {RAISE: "raise", WRAP: "wrap", CLIP: "clip"}
X, Y, Z, AXIS, UNBOUNDED, QUAT, FREEFLYER, PX = 1, 2, 3, 4, 5, 6, 7, 8
# designed lanes of `anymal`, event 0
LANES = ("on_sample", "below_sample", "doubled", "t_start", "t_end", "beyond_raise", "beyond_clip", "beyond_wrap", "beyond_wrap3",
         "before_raise", "before_clip", "before_wrap", "stride_yaw", "stride_zero", "degenerate_wrap", "pair_2.5rad", "pair_1e-9rad")


def load_reference_definitions(extra: dict) -> dict:
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    ns: dict = {"np": np, "nb": nb, "math": math, "ArrayOrScalar": typing.Any, "dataclass": dataclass, "fields": fields,
                "bisect_left": bisect_left}
    ns.update({k: getattr(typing, k) for k in ("Optional", "Tuple", "Union", "List", "Sequence", "Dict", "Literal", "overload",
                                               "no_type_check", "Callable")})
    ns.update(extra)
    for path, names in SOURCES.items():
        with open(path) as f:
            tree = ast.parse(f.read(), filename=path)
        found = set()
        for node in tree.body:
            name = None
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
                name = node.name
            elif isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and \
                    node.targets[0].id in names:
                name = node.targets[0].id
            if name is not None:      # (typing overloads first, the definition last)
                exec(compile(ast.Module([node], []), path, "exec"), ns)
                found.add(name)
        if set(names) - found:
            raise RuntimeError(f"{path}: {sorted(set(names) - found)} not found")
    return ns


# ------------------------------------------------------------------------------------------------------ restated stand-ins
class Robot:
    """RESTATED: what `Trajectory` reads of a `jiminy.Robot`: `has_freeflyer` and a model, here the joint table."""

    def __init__(self, joint_kind, joint_q_index) -> None:
        self.joints = [(int(k), int(r)) for k, r in zip(joint_kind, joint_q_index)]
        self.has_freeflyer = bool(self.joints) and self.joints[0][0] == FREEFLYER
        self.pinocchio_model = self.pinocchio_model_th = self


def make_pin(ns: dict) -> types.SimpleNamespace:
    """RESTATED: the part of pinocchio `Trajectory` calls, on the reference's own `quat_multiply`, `quat_apply`, `log3`, `exp3`,
    `log6`, `exp6` (filled in once they are loaded: `ns` is the namespace they live in)."""

    class SE3:
        def __init__(self, xyzquat) -> None:
            self.xyzquat = np.array(xyzquat, dtype=np.float64)

        def __mul__(self, other: "SE3") -> "SE3":
            pos = self.xyzquat[:3] + ns["quat_apply"](self.xyzquat[3:], other.xyzquat[:3])
            return SE3(np.concatenate((pos, ns["quat_multiply"](self.xyzquat[3:], other.xyzquat[3:]))))

        def inverse(self) -> "SE3":
            quat = self.xyzquat[3:] * np.array([-1.0, -1.0, -1.0, 1.0])
            return SE3(np.concatenate((-ns["quat_apply"](quat, self.xyzquat[:3]), quat)))

    def interpolate(model: Robot, q0: np.ndarray, q1: np.ndarray, alpha: float) -> np.ndarray:
        out = np.empty_like(q0)
        for kind, row in model.joints:
            if kind == FREEFLYER:
                M0, M1 = SE3(q0[row:row + 7]), SE3(q1[row:row + 7])
                out[row:row + 7] = (M0 * SE3(ns["exp6"](alpha * ns["log6"]((M0.inverse() * M1).xyzquat)))).xyzquat
            elif kind == QUAT:
                delta = ns["quat_multiply"](q0[row:row + 4], q1[row:row + 4], None, True, False)
                out[row:row + 4] = ns["quat_multiply"](q0[row:row + 4], ns["exp3"](alpha * ns["log3"](delta)))
            elif kind == UNBOUNDED:
                c0, s0, c1, s1 = q0[row], q0[row + 1], q1[row], q1[row + 1]
                angle = alpha * np.arctan2(c0 * s1 - s0 * c1, c0 * c1 + s0 * s1)
                out[row], out[row + 1] = c0 * np.cos(angle) - s0 * np.sin(angle), s0 * np.cos(angle) + c0 * np.sin(angle)
            else:
                out[row] = q0[row] + alpha * (q1[row] - q0[row])
        return out

    return types.SimpleNamespace(
        SE3=SE3, XYZQUATToSE3=SE3, SE3ToXYZQUAT=lambda M: M.xyzquat.copy(), interpolate=interpolate,
        log6=lambda M: ns["log6"](M.xyzquat), exp6=lambda v: SE3(ns["exp6"](np.asarray(v, dtype=np.float64))))


def select_offset(time_interval, ratio: float) -> float:
    """RESTATED: `DatasetTrajectoryQuantity._select` (bases/quantities.py:1171-1174)."""
    t_start, t_end = time_interval
    return t_start + ratio * (t_end - t_start)


def odom_pose(ref: dict, q: np.ndarray) -> np.ndarray:
    """RESTATED: `BaseOdometryPose.refresh` (quantities/locomotion.py:211-219) on the reference's `quat_to_yaw`."""
    return np.array([q[0], q[1], float(ref["quat_to_yaw"](q[3:7]))])


# ------------------------------------------------------------------------------------------------------------ the datasets
def grid(rg, size, scale: float = 1.0) -> np.ndarray:
    return np.round(rg.uniform(-scale, scale, size=size) * GRID) / GRID


def unit(v: np.ndarray) -> np.ndarray:
    return v / np.linalg.norm(v)


def rotation_quat(axis: np.ndarray, angle: float) -> np.ndarray:
    axis = unit(np.asarray(axis, dtype=np.float64))
    return np.concatenate((np.sin(angle / 2) * axis, [np.cos(angle / 2)]))


def quat_product(l: np.ndarray, r: np.ndarray) -> np.ndarray:
    return unit(np.array([l[3] * r[0] + l[0] * r[3] + l[1] * r[2] - l[2] * r[1], l[3] * r[1] - l[0] * r[2] + l[1] * r[3] + l[2] * r[0],
                          l[3] * r[2] + l[0] * r[1] - l[1] * r[0] + l[2] * r[3], l[3] * r[3] - l[0] * r[0] - l[1] * r[1] - l[2] * r[2]]))


def quat_walk(rg, n: int, angles=None) -> np.ndarray:
    """n unit quaternions, each the previous one turned by less than a radian (or by `angles[k]` before sample k): consecutive
    dot products are positive."""
    out = [rotation_quat(rg.normal(size=3), rg.uniform(0.1, 0.6))]
    for k in range(1, n):
        angle = rg.uniform(0.05, 0.5) if angles is None or angles.get(k) is None else angles[k]
        step = rotation_quat(rg.normal(size=3), angle)
        out.append(quat_product(out[-1], step))
    out = np.array(out)
    assert np.all(np.sum(out[1:] * out[:-1], axis=1) > 0)
    return out


def quat_yaw_walk(rg, n: int, total_yaw: float) -> np.ndarray:
    """n unit quaternions turning about the vertical by `total_yaw` in equal steps, each tilted by a small rotation of its own;
    the last one is exactly the first one turned by `total_yaw`: the stride is that yaw."""
    base = rotation_quat(rg.normal(size=3), 0.2)
    tilt = [rotation_quat(rg.normal(size=3), rg.uniform(0.02, 0.15)) for _ in range(n - 1)]
    tilt.append(tilt[0])
    out = np.array([quat_product(rotation_quat([0, 0, 1], total_yaw * k / (n - 1)), quat_product(base, tilt[k])) for k in range(n)])
    assert np.all(np.sum(out[1:] * out[:-1], axis=1) > 0)
    return out


def draw_samples(rg, table, times, widths, angles=None, closed: bool = False, total_yaw: float = 0.0) -> np.ndarray:
    """`[S][R]`: q by joint kind, then the other fields (`widths`: their row counts) on the grid."""
    n = len(times)
    nq = max(row + {FREEFLYER: 7, QUAT: 4, UNBOUNDED: 2}.get(kind, 1) for kind, row in table)
    q = np.zeros((n, nq))
    for kind, row in table:
        if kind == FREEFLYER:
            q[:, row:row + 3] = grid(rg, (n, 3), 2.0)
            q[:, row + 3:row + 7] = quat_yaw_walk(rg, n, total_yaw) if total_yaw else quat_walk(rg, n, angles)
        elif kind == QUAT:
            q[:, row:row + 4] = quat_walk(rg, n, angles)
        elif kind == UNBOUNDED:
            angle = np.cumsum(rg.uniform(-1.2, 1.2, size=n))
            q[:, row], q[:, row + 1] = np.cos(angle), np.sin(angle)
        else:
            q[:, row] = grid(rg, n, 1.5)
    if closed:
        q[-1] = q[0]
    return np.concatenate([q] + [grid(rg, (n, w), 3.0) for w in widths], axis=1)


def g(*values) -> np.ndarray:
    out = np.array(values, dtype=np.float64)
    assert np.all(out * GRID == np.round(out * GRID))
    return out


TIMES_2 = g(0.5, 1.25)
TIMES_5 = g(1.0, 1.25, 1.75, 1.75, 2.5)                       # (samples 2 and 3: t-, t+)
TIMES_9 = g(0.25, 0.5, 0.5625, 1.0, 1.25, 1.75, 1.8125, 2.5, 3.0)
TIMES_6 = g(-1.0, -0.5, 0.0, 0.125, 1.0, 1.5)
PAIR_BIG, PAIR_SMALL = 1, 4                                     # (right samples of the 2.5 rad and of the 1e-9 rad pair of TIMES_5)


def dataset_anymal(rg) -> dict:
    table = [(FREEFLYER, 0)] + [(X + (j % 3), 7 + j) for j in range(12)]
    widths = (18, 12)                                            # v, command
    shapes = [(TIMES_2, draw_samples(rg, table, TIMES_2, widths)),
              (TIMES_5, draw_samples(rg, table, TIMES_5, widths, angles={PAIR_BIG: 2.5, PAIR_SMALL: 1e-9})),
              (TIMES_9, draw_samples(rg, table, TIMES_9, widths, total_yaw=1.0))]
    entries = [(t, d, mode) for t, d in shapes for mode in (RAISE, WRAP, CLIP)]
    entries.append((TIMES_5, draw_samples(rg, table, TIMES_5, widths, closed=True), WRAP))        # stride 0
    entries.append((g(0.75, 0.75), draw_samples(rg, table, g(0.75, 0.75), widths), WRAP))         # t_end == t_start
    return pack_dataset(table, entries, nv=18, n_command=12, fields=tn.HAS_V | tn.HAS_COMMAND, motors=list(range(7, 19)))


def dataset_mixed(rg) -> dict:
    table = [(FREEFLYER, 0), (QUAT, 7), (UNBOUNDED, 11), (PX, 13), (Y, 14)]
    widths = (12, 12)                                            # v, a
    entries = [(TIMES_6, draw_samples(rg, table, TIMES_6, widths), mode) for mode in (RAISE, WRAP, CLIP)]
    entries.append((TIMES_2, draw_samples(rg, table, TIMES_2, widths), WRAP))
    return pack_dataset(table, entries, nv=12, n_command=2, fields=tn.HAS_V | tn.HAS_A, motors=[13, 14])


def dataset_fixed(rg) -> dict:
    table = [(Z, 0), (X, 1), (AXIS, 2), (UNBOUNDED, 3)]
    entries = [(TIMES_6, draw_samples(rg, table, TIMES_6, ()), mode) for mode in (RAISE, WRAP, CLIP)]
    return pack_dataset(table, entries, nv=4, n_command=3, fields=0, motors=[0, 1, 2])


def pack_dataset(table, entries, *, nv, n_command, fields, motors) -> dict:
    nq = max(row + {FREEFLYER: 7, QUAT: 4, UNBOUNDED: 2}.get(kind, 1) for kind, row in table)
    start = np.cumsum([0] + [len(t) for t, _, _ in entries]).astype(np.int32)
    return {"sample_start": start, "times": np.concatenate([t for t, _, _ in entries]),
            "mode": np.array([m for _, _, m in entries], dtype=np.int32), "data": np.concatenate([d for _, d, _ in entries], axis=0),
            "nq": np.int32(nq), "nv": np.int32(nv), "n_command": np.int32(n_command), "fields": np.int32(fields),
            "joint_kind": np.array([k for k, _ in table], dtype=np.int32), "joint_q_index": np.array([r for _, r in table], dtype=np.int32),
            "motor_q_index": np.array(motors, dtype=np.int32)}


# ---------------------------------------------------------------------------------------------------------- the reference
def reference_trajectories(ref: dict, plan: dict) -> list:
    """One `Trajectory` of the reference per trajectory of the plan, on the robot stand-in."""
    robot = Robot(plan["joint_kind"], plan["joint_q_index"])
    nq, nv, fields_ = int(plan["nq"]), int(plan["nv"]), int(plan["fields"])
    out = []
    for k in range(len(plan["mode"])):
        states = []
        for s in range(plan["sample_start"][k], plan["sample_start"][k + 1]):
            row, first, extra = plan["data"][s], nq, {}
            for name, bit, width in (("v", tn.HAS_V, nv), ("a", tn.HAS_A, nv), ("command", tn.HAS_COMMAND, int(plan["n_command"]))):
                if fields_ & bit:
                    extra[name] = row[first:first + width].copy()
                    first += width
            states.append(ref["State"](t=float(plan["times"][s]), q=row[:nq].copy(), **extra))
        out.append(ref["Trajectory"](states, robot, False))
    return out


def run_case(ref: dict, plan: dict, events: dict) -> dict:
    """`Trajectory.get` lane by lane, event by event, with the carry-over of the lanes an event leaves out."""
    trajectories = reference_trajectories(ref, plan)
    if tn.has_freeflyer(plan):
        plan["stride"] = np.array([t._stride_offset_log6 for t in trajectories])
    names = [n for n in tn.OUTPUTS if tn.rows_of(n, plan)]
    held = {n: np.zeros((tn.rows_of(n, plan), B), dtype=np.int32 if n == "status" else np.float64) for n in names}
    expected = {n: [] for n in names}
    motors = np.asarray(plan["motor_q_index"], dtype=np.int64)
    for e in range(events["time"].shape[0]):
        for b in np.flatnonzero(events["mask"][e]):
            k, mode = int(events["trajectory"][e, b]), int(plan["mode"][int(events["trajectory"][e, b])])
            traj = trajectories[k]
            t = float(events["time"][e, b]) + float(events["time_offset"][e, b])
            flags = 0
            try:
                state = traj.get(t, MODE_NAMES[mode])
            except RuntimeError:
                # (the device cannot raise: the flag, then the state at the clipped time)
                flags = 1
                state = traj.get(t, "clip")
            t_start, t_end = traj.time_interval
            n_steps = int(divmod(t - t_start, t_end - t_start)[0]) if mode == WRAP and t_end > t_start else 0
            held["status"][:, b] = (flags, n_steps, traj._index_prev)
            held["q"][:, b] = state.q
            for name in ("v", "a", "command"):
                if name in held:
                    held[name][:, b] = getattr(state, name)
            if "odom_pose" in held:
                held["odom_pose"][:, b] = odom_pose(ref, state.q)
            if "position" in held:
                held["position"][:, b] = state.q[motors]
        for n in names:
            expected[n].append(held[n].copy())
    return {n: np.stack(v) for n, v in expected.items()}


# --------------------------------------------------------------------------------------------------------------- the queries
def mapped_time(plan: dict, k: int, t: float) -> float:
    s0, s1 = int(plan["sample_start"][k]), int(plan["sample_start"][k + 1])
    t_start, t_end = float(plan["times"][s0]), float(plan["times"][s1 - 1])
    if int(plan["mode"][k]) == WRAP:
        return divmod(t - t_start, t_end - t_start)[1] + t_start if t_end > t_start else t_start
    return min(max(t, t_start), t_end)


def apart(plan: dict, k: int, t: float) -> bool:
    """The drawing condition: the mapped time is at least one grid step from its two neighbours, or the query lies outside the
    trajectory in mode raise or clip (it is clipped onto the first or the last sample)."""
    s0, s1 = int(plan["sample_start"][k]), int(plan["sample_start"][k + 1])
    if int(plan["mode"][k]) != WRAP and not float(plan["times"][s0]) <= t <= float(plan["times"][s1 - 1]):
        return True
    tm, t = plan["times"][s0:s1], mapped_time(plan, k, t)
    i = bisect_left(list(tm), t, 1, len(tm) - 1)
    return t - tm[i - 1] >= 1 / GRID and tm[i] - t >= 1 / GRID


def draw_events(rg, plan: dict, n_events: int, designed=None, masked_event=None) -> dict:
    N = len(plan["mode"])
    ev = {"time": np.zeros((n_events, B)), "trajectory": np.zeros((n_events, B), dtype=np.int32),
          "time_offset": np.zeros((n_events, B)), "mask": np.ones((n_events, B), dtype=bool)}
    for e in range(n_events):
        if e == masked_event:
            ev["mask"][e] = rg.uniform(size=B) < 0.5
            assert ev["mask"][e].any() and not ev["mask"][e].all()
        for b in range(B):
            if e == 0 and designed is not None and b < len(designed):
                k, time, ratio = designed[b]
            else:
                while True:
                    k = int(rg.integers(N))
                    s0, s1 = int(plan["sample_start"][k]), int(plan["sample_start"][k + 1])
                    t_start, t_end = float(plan["times"][s0]), float(plan["times"][s1 - 1])
                    span = max(t_end - t_start, 0.5)
                    ratio = float(np.round(rg.uniform(0.0, 1.0) * 16) / 16)
                    offset = select_offset((t_start, t_end), ratio)
                    t = float(np.round(rg.uniform(t_start - 1.5 * span, t_end + 3.5 * span) * GRID) / GRID)
                    time = t - offset
                    if time + offset == t and (t_end == t_start or apart(plan, k, t)):
                        break
            s0, s1 = int(plan["sample_start"][k]), int(plan["sample_start"][k + 1])
            ev["trajectory"][e, b], ev["time"][e, b] = k, time
            ev["time_offset"][e, b] = select_offset((float(plan["times"][s0]), float(plan["times"][s1 - 1])), ratio)
    return ev


def designed_anymal(plan: dict) -> list:
    """(trajectory, lane time, offset ratio) of the designed lanes, in the order of LANES.  Trajectories of `dataset_anymal`:
    0-2 two samples, 3-5 five samples, 6-8 nine samples (raise, wrap, clip each), 9 closed (wrap), 10 degenerate (wrap)."""
    t9, span9 = TIMES_9, TIMES_9[-1] - TIMES_9[0]

    def at(k: int, t: float):           # ratio 0: the offset is t_start
        s0 = int(plan["sample_start"][k])
        return (k, t - float(plan["times"][s0]), 0.0)

    return [at(8, t9[3]), at(8, t9[3] - 2.0 ** -40), at(5, TIMES_5[2]), at(6, t9[0]), at(6, t9[-1]),
            at(6, t9[-1] + 0.25), at(8, t9[-1] + 0.25), at(7, t9[-1] + 0.125), at(7, t9[0] + 3 * span9 + 0.125),
            at(6, t9[0] - 0.25), at(8, t9[0] - 0.25), at(7, t9[0] - 0.125), at(7, t9[0] + 3 * span9 + 1.0),
            at(9, TIMES_5[-1] + 0.5), at(10, 2.0), at(5, 0.5 * (TIMES_5[PAIR_BIG - 1] + TIMES_5[PAIR_BIG])),
            at(5, 0.5 * (TIMES_5[PAIR_SMALL - 1] + TIMES_5[PAIR_SMALL]))]


def check_designed(plan: dict, events: dict, expected: dict) -> None:
    lane = {name: b for b, name in enumerate(LANES)}
    status, q, data, nq = expected["status"][0], expected["q"][0], plan["data"], int(plan["nq"])
    sample = lambda k, i: data[int(plan["sample_start"][k]) + i, :nq]       # noqa: E731
    flags, n_steps, index = status
    assert index[lane["on_sample"]] == 3 and np.array_equal(q[:, lane["on_sample"]], sample(8, 3))
    assert index[lane["below_sample"]] == 3 and np.array_equal(q[:, lane["below_sample"]], sample(8, 3))
    assert index[lane["doubled"]] == 2 and np.array_equal(q[:, lane["doubled"]], sample(5, 2))          # t-, the left one
    assert index[lane["t_start"]] == 1 and np.array_equal(q[:, lane["t_start"]], sample(6, 0))
    assert index[lane["t_end"]] == 8 and np.array_equal(q[:, lane["t_end"]], sample(6, 8))
    assert flags[lane["beyond_raise"]] == 1 and np.array_equal(q[:, lane["beyond_raise"]], sample(6, 8))
    assert flags[lane["before_raise"]] == 1 and np.array_equal(q[:, lane["before_raise"]], sample(6, 0))
    assert flags[lane["beyond_clip"]] == 0 and np.array_equal(q[:, lane["beyond_clip"]], sample(8, 8))
    assert flags[lane["before_clip"]] == 0 and np.array_equal(q[:, lane["before_clip"]], sample(8, 0))
    assert [int(n_steps[lane[n]]) for n in ("beyond_wrap", "beyond_wrap3", "before_wrap", "stride_yaw", "stride_zero")] == [1, 3, -1, 3, 1]
    assert int(flags.sum()) == 2 + int(np.sum(flags[len(LANES):]))
    stride = plan["stride"]
    assert 0.9 < abs(stride[7, 5]) < 1.1 and np.all(np.abs(stride[9]) < 1e-15)       # (the reference's products leave 1e-16)
    # the closed trajectory: odometry with a zero stride leaves the interpolated state as it is
    assert n_steps[lane["stride_zero"]] == 1 and np.all(np.isfinite(q[:, lane["stride_zero"]]))
    assert n_steps[lane["degenerate_wrap"]] == 0 and np.array_equal(q[:, lane["degenerate_wrap"]], sample(10, 0))
    quat = lambda k, i: sample(k, i)[3:7]       # noqa: E731
    angle = lambda a, b: 2 * np.arccos(min(1.0, abs(float(np.dot(a, b)))))       # noqa: E731
    assert abs(angle(quat(5, PAIR_BIG - 1), quat(5, PAIR_BIG)) - 2.5) < 1e-6
    assert index[lane["pair_2.5rad"]] == PAIR_BIG and index[lane["pair_1e-9rad"]] == PAIR_SMALL
    small = quat(5, PAIR_SMALL - 1) - quat(5, PAIR_SMALL)
    assert 1e-10 < np.linalg.norm(small) < 1e-9


def check_dataset(plan: dict) -> None:
    nq = int(plan["nq"])
    for k in range(len(plan["mode"])):
        q = plan["data"][plan["sample_start"][k]:plan["sample_start"][k + 1], :nq]
        for kind, row in zip(plan["joint_kind"], plan["joint_q_index"]):
            if kind in (FREEFLYER, QUAT):
                quat = q[:, row + 3:row + 7] if kind == FREEFLYER else q[:, row:row + 4]
                assert np.all(np.sum(quat[1:] * quat[:-1], axis=1) > 0)


def pack_case(plan: dict, events: dict, expected: dict) -> dict:
    out = {f"plan.{k}": np.asarray(v) for k, v in plan.items() if v is not None}
    out.update({k: np.asarray(v) for k, v in events.items()})
    out.update({f"expected.{k}": v for k, v in expected.items()})
    return out


def make_cases(ref: dict, rg) -> dict:
    out = {}
    plan = dataset_anymal(rg)
    check_dataset(plan)
    events = draw_events(rg, plan, 4, designed=designed_anymal(plan), masked_event=2)
    expected = run_case(ref, plan, events)
    check_designed(plan, events, expected)
    out["anymal"] = pack_case(plan, events, expected)
    for label, make in (("mixed", dataset_mixed), ("fixed", dataset_fixed)):
        plan = make(rg)
        check_dataset(plan)
        events = draw_events(rg, plan, 3, masked_event=1)
        expected = run_case(ref, plan, events)
        if label == "fixed":
            assert "stride" not in plan and "odom_pose" not in expected and np.any(expected["status"][:, 1] != 0)
        out[label] = pack_case(plan, events, expected)
    return out


def main(out_path: str, verbose: bool = True) -> None:
    ns: dict = {}
    pin = make_pin(ns)
    ns.update(load_reference_definitions({"pin": pin, "jiminy": types.SimpleNamespace(Robot=Robot, Model=Robot)}))
    assert ns["TRAJ_INTERP_TOL"] == tn.TOL
    rg = np.random.default_rng(SEED)
    out: dict = {}
    cases = make_cases(ns, rg)
    for label, case in cases.items():
        for k, v in case.items():
            out[f"{label}.{k}"] = v
    out["cases"] = np.array(list(cases))
    out["designed_lanes"] = np.array(LANES)
    out["tier"] = np.array("A: the reference's State, Trajectory.__init__ / time_interval / get and TRAJ_INTERP_TOL, on its log6, exp6, "
                           "log3, exp3, quat_multiply, quat_apply, quat_to_yaw; the pin and robot stand-ins, _select's offset and "
                           "BaseOdometryPose.refresh are restated")
    np.savez_compressed(out_path, **out)
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")
    assert os.path.getsize(out_path) < 500e3


if __name__ == "__main__":
    if not os.path.isfile(DYNAMICS):
        sys.exit(f"{DYNAMICS} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            fresh = os.path.join(tmp, "ref_trajectory.npz")
            main(fresh, verbose=False)
            same = open(fresh, "rb").read() == open(OUT, "rb").read()
        print("tests/golden/ref_trajectory.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
