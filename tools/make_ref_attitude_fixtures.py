"""Reference-pinned fixtures of the attitude observers (MahonyFilter with its options, BodyObserver): EXECUTES THE
REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_deformation_fixtures.py: this script parses the reference files where they lie,
takes the function definitions named in SOURCES (decorators included) and executes them with `numba.jit` stubbed to the
identity.  Nothing of the reference is copied into the repository: only authored descriptions, seeded inputs and the
outputs the reference's code produced for them, written to tests/golden/ref_attitude.npz.

Run where the reference tree is available:   python tools/make_ref_attitude_fixtures.py [output.npz]

Tier A for the functions, a restated composition for the glue: every number comes out of the reference's functions
(`mahony_filter`, `update_twist`, `compute_tilt_from_quat`, `swing_from_vector`, `remove_twist_from_quat`, `quat_to_rpy`,
`quat_multiply`, `quat_apply`, `matrices_to_quat`) called on the arrays they are written for, one environment at a time.
What this script restates is the ORDER in which the two classes' `refresh_observation` bodies call them
(blocks/mahony_filter.py:337-393, blocks/body_orientation_observer.py:237-266), the accelerometer test and normalisation
of the initialisation (:342, :352) and, for the exact initialisation, the frame rotations handed to `matrices_to_quat`
(numpy products of the authored segments, where the reference reads pinocchio).

Every case holds 64 lanes and (but the initialisation) 5 consecutive ticks: the state carries over.  Lanes are drawn away
from discontinuities and redrawn otherwise, so that every stored lane counts: within 1e-3 of a branch test of
`matrices_to_quat` or of the +-pi cut of roll / yaw, within a factor 2 of a narrow threshold (1e-5 of `swing_from_vector`,
1e-6 of the filter's early return, 0.1 g of the initialisation), pitch within 1e-2 of +-pi/2.  `swing_from_vector` loses
1 / (1 + v_z) digits in its regular branch: outside the ticks authored as singular every tilt keeps v_z >= -0.95.
Inputs that need no more are float32 values (the archive stays small); attitudes are full float64.
"""
from __future__ import annotations

import ast
import json
import os
import sys
import types
import typing

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_ref_deformation_fixtures as mdf     # noqa: E402  (authored helpers: rotations, branch names, margins)

REF = os.environ.get("JIMINY_REFERENCE", "/root/reference")
COMMON = os.path.join(REF, "python/gym_jiminy/common/gym_jiminy/common")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_attitude.npz")

SOURCES = {
    "utils/math.py": ("compute_tilt_from_quat", "swing_from_vector", "remove_twist_from_quat", "quat_to_rpy", "quat_multiply",
                      "quat_apply", "matrices_to_quat"),
    "blocks/mahony_filter.py": ("mahony_filter",),
    "blocks/body_orientation_observer.py": ("update_twist",),
}
B = 64
TICKS = 5
SEED = 20261017
G = 9.81
VZ_MIN = -0.95
SEG_NONE, SEG_X, SEG_Y, SEG_Z, SEG_AXIS, SEG_UNBOUNDED, SEG_QUAT = range(7)
SINGULAR_KINDS = ("xy", "ratio_x", "ratio_y", "general_x", "general_y")


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
        for node in tree.body:      # module-level constants (TWIST_SWING_SINGULAR_THR, EARTH_SURFACE_GRAVITY)
            if isinstance(node, ast.Assign) and all(isinstance(t, ast.Name) for t in node.targets) \
                    and isinstance(node.value, ast.Constant):
                exec(compile(ast.Module([node], []), path, "exec"), ns)
        found = set()
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and node.name in names:      # (typing overloads first, the definition last)
                exec(compile(ast.Module([node], []), path, "exec"), ns)
                found.add(node.name)
        if set(names) - found:
            raise RuntimeError(f"{rel}: functions {sorted(set(names) - found)} not found")
    return ns


def f32(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def upright_quat(rg: np.random.Generator, max_tilt: float = 1.0) -> np.ndarray:
    """Any yaw after a tilt of at most `max_tilt` rad about a horizontal-ish random axis."""
    return mdf.qmul(mdf.quat_axis_angle(np.array([0.0, 0.0, 1.0]), rg.uniform(-np.pi, np.pi)),
                    mdf.quat_axis_angle(mdf.random_unit(rg), rg.uniform(-max_tilt, max_tilt)))


def rpy_ok(e: np.ndarray, skip_cut=()) -> bool:
    ok = bool(np.isfinite(e).all() and (np.abs(e[1]) <= np.pi / 2 - mdf.PITCH_MARGIN).all())
    for s in range(e.shape[1]):
        if s not in skip_cut:
            ok &= bool((np.abs(e[[0, 2], s]) <= np.pi - mdf.RPY_MARGIN).all())
    return ok


# --------------------------------------------------------------------------------------------------------- Mahony cases
def mahony_lane(ref, rg, n_imu, kp, ki, dt, ignore_twist, compute_rpy, kind, singular):
    """One lane over TICKS ticks.  kind: 'move' | 'rest' (every IMU at rest on ticks 0, 1, 3) | 'one' (only IMU 1 moves: the others
    turn by 1e-8 rad/s) |
    'singular' (IMU `lane-chosen` upside down in branch `singular` and the lane at rest on tick 0, then it is turned away).
    Returns None when a margin is not kept."""
    quat = np.stack([upright_quat(rg) for _ in range(n_imu)], 1)
    which = int(rg.integers(n_imu)) if kind == "singular" else -1
    if which >= 0:
        quat[:, which] = mdf.quat_with_tilt(rg, mdf.singular_tilt(rg, singular))
    bias = f32(rg.normal(scale=0.01, size=(3, n_imu)))
    omega, cf, rpy = np.zeros((3, n_imu)), np.zeros((3, n_imu)), np.zeros((3, n_imu))
    rec = dict(quat0=quat.copy(), bias0=bias.copy(), imu=[], quat=[], bias=[], rpy=[], omega=None, cf=None)
    hits = {"rest": 0, "moving": 0, "swing": {}}
    away = mdf.random_unit(rg) * np.array([1.0, 1.0, 0.0])
    away /= np.linalg.norm(away)
    for t in range(TICKS):
        tilt = np.stack(ref["compute_tilt_from_quat"](quat))           # [3][n_imu]
        gyro, acc = np.zeros((3, n_imu)), np.zeros((3, n_imu))
        for s in range(n_imu):
            at_rest = (kind == "rest" and t in (0, 1, 3)) or (kind == "one" and s != 1) or (kind == "singular" and t == 0)
            if at_rest:
                gyro[:, s], acc[:, s] = bias[:, s], f32(G * rg.uniform(0.8, 1.2) * tilt[:, s])
                if kind == "one":
                    # next to a moving IMU the filter divides the correction of a resting one by its norm: a rate of 1e-8
                    # rad/s, a hundredth of the filter's threshold, keeps that norm away from zero in float32 as well
                    gyro[:, s] += rg.choice([-1.0, 1.0], 3) * rg.uniform(1e-8, 3e-8, 3)
            elif s == which:
                gyro[:, s], acc[:, s] = f32(bias[:, s] + 40.0 * away), f32(G * tilt[:, s] + rg.normal(scale=1.0, size=3))
            else:
                gyro[:, s], acc[:, s] = f32(rg.normal(scale=1.0, size=3)), f32(G * tilt[:, s] + rg.normal(scale=2.0, size=3))
        ref["mahony_filter"](quat, omega, cf, gyro, acc, bias, kp, ki, dt)
        resting, moving = bool((np.abs(cf) < 5e-7).all()), bool((np.abs(cf) > 2e-6).any())
        if resting == moving or resting != (kind in ("rest", "singular") and (t == 0 or (kind == "rest" and t in (1, 3)))):
            return None
        hits["rest" if resting else "moving"] += 1
        if ignore_twist:
            tilt = np.stack(ref["compute_tilt_from_quat"](quat))
            for s in range(n_imu):
                name, keeps = mdf.swing_branch(tilt[:, s])
                want = singular if (s == which and t == 0) else "regular"
                if name != want or not keeps or (want == "regular" and tilt[2, s] < VZ_MIN):
                    return None
                hits["swing"][name] = hits["swing"].get(name, 0) + 1
            ref["remove_twist_from_quat"](quat)
        if compute_rpy:
            ref["quat_to_rpy"](quat, rpy)
            if not rpy_ok(rpy, skip_cut=(which,) if t == 0 else ()):
                return None
        if not (np.isfinite(quat).all() and np.isfinite(bias).all()):
            return None
        rec["imu"].append(np.concatenate([gyro, acc], 0).T.copy())      # [n_imu][6]
        rec["quat"].append(quat.copy()); rec["bias"].append(bias.copy()); rec["rpy"].append(rpy.copy())
    rec["omega"], rec["cf"] = omega.copy(), cf.copy()
    return rec, hits


def mahony_case(ref, rg, n_imu, ignore_twist, compute_rpy, kinds, dt=0.005, singular=False):
    kp = f32(rg.uniform(0.5, 2.0, n_imu))
    ki = f32(rg.uniform(0.05, 0.3, n_imu))
    lanes, total, rejected = [], {"rest": 0, "moving": 0, "swing": {}}, 0
    lane_kind = []
    while len(lanes) < B:
        kind = kinds[len(lanes) % len(kinds)]
        branch = SINGULAR_KINDS[(len(lanes) // len(kinds)) % len(SINGULAR_KINDS)] if kind == "singular" else ""
        got = mahony_lane(ref, rg, n_imu, kp, ki, dt, ignore_twist, compute_rpy, kind, branch)
        if got is None:
            rejected += 1
            if rejected > 400 * B:
                raise RuntimeError("too many rejected lanes")
            continue
        rec, hits = got
        lanes.append(rec)
        lane_kind.append(kind + (":" + branch if branch else ""))
        for k in ("rest", "moving"):
            total[k] += hits[k]
        for k, v in hits["swing"].items():
            total["swing"][k] = total["swing"].get(k, 0) + v
    stack = lambda key: np.stack([np.stack(r[key]) for r in lanes], -1)     # noqa: E731  [T][...][B]
    case = dict(n_imu=np.int32(n_imu), kp=kp, ki=ki, dt=np.float64(dt), ignore_twist=np.int32(ignore_twist),
                compute_rpy=np.int32(compute_rpy), quat0=np.stack([r["quat0"] for r in lanes], -1),
                bias0=np.stack([r["bias0"] for r in lanes], -1), imu=stack("imu"), quat=stack("quat"),
                bias=np.stack([r["bias"][-1] for r in lanes], -1),      # (state and scratch outputs: after the last tick)
                omega=np.stack([r["omega"] for r in lanes], -1), cf=np.stack([r["cf"] for r in lanes], -1),
                lane_kind=np.array(lane_kind), hits=np.array(json.dumps(total, sort_keys=True)))
    if compute_rpy:
        case["rpy"] = stack("rpy")
    return case, rejected


# ------------------------------------------------------------------------------------------------- initialisation case
def init_description():
    """Three IMU frames behind every kind of joint: a free-flyer orientation, revolute joints about x / y / z and about a
    skew axis, an unbounded revolute joint (cos, sin), a spherical joint; constant rotations in between."""
    axis_a, axis_b = np.array([0.6, 0.0, 0.8]), np.array([2.0, -1.0, 2.0]) / 3.0
    frames = [
        [((0.0, 0.0, 0.0), SEG_QUAT, 3, None), ((0.3, -0.2, 1.1), SEG_NONE, -1, None)],
        [((0.0, 0.0, 0.0), SEG_QUAT, 3, None), ((1.9, -0.7, 2.4), SEG_X, 7, None), ((-0.4, 0.5, 0.2), SEG_AXIS, 8, axis_a),
         ((2.8, 0.2, -1.0), SEG_NONE, -1, None)],
        [((0.0, 0.0, 0.0), SEG_QUAT, 3, None), ((0.1, 0.2, -0.3), SEG_Z, 9, None), ((-2.6, 0.9, 0.8), SEG_UNBOUNDED, 10, axis_b),
         ((0.2, 0.0, 0.0), SEG_QUAT, 12, None), ((0.0, 1.2, 0.0), SEG_Y, 16, None)],
    ]
    start, kind, qi, rot, axis = [0], [], [], [], []
    for segs in frames:
        for rpy_, k, i, a in segs:
            kind.append(k); qi.append(i); rot.append(mdf.rot_rpy(*rpy_)); axis.append(np.zeros(3) if a is None else a)
        start.append(len(kind))
    return dict(nq=np.int32(17), frame_seg_start=np.asarray(start, np.int32), seg_kind=np.asarray(kind, np.int32),
                seg_q_index=np.asarray(qi, np.int32), seg_rot=np.array(rot), seg_axis=np.array(axis))


def quat_rot(q: np.ndarray) -> np.ndarray:
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def frame_rotation(d: dict, s: int, q: np.ndarray) -> np.ndarray:
    R = np.eye(3)
    for g in range(d["frame_seg_start"][s], d["frame_seg_start"][s + 1]):
        R = R @ d["seg_rot"][g]
        k, i = int(d["seg_kind"][g]), int(d["seg_q_index"][g])
        if k in (SEG_X, SEG_Y, SEG_Z, SEG_AXIS):
            R = R @ mdf.rot_axis_angle(d["seg_axis"][g] if k == SEG_AXIS else np.eye(3)[k - 1], q[i])
        elif k == SEG_UNBOUNDED:
            R = R @ mdf.rot_axis_angle(d["seg_axis"][g], np.arctan2(q[i + 1], q[i]))
        elif k == SEG_QUAT:
            R = R @ quat_rot(q[i:i + 4])
    return R


def init_case(ref, rg):
    d = init_description()
    n_imu, low = 3, 0.1 * G
    q_all, imu_all, exact, acc_q, rpy_e, rpy_a, kinds = [], [], [], [], [], [], []
    m2q_hits, swing_hits, rejected = np.zeros(4, dtype=np.int64), {}, 0
    while len(q_all) < B:
        lane_kind = ("regular", "fallback", "single")[len(q_all) % 3]
        q = rg.normal(size=17)
        q[3:7] = mdf.qmul(mdf.quat_axis_angle(mdf.random_unit(rg), rg.uniform(-3.0, 3.0)), np.array([0, 0, 0, 1.0]))
        q[7:10] = rg.uniform(-2.5, 2.5, 3)
        a = rg.uniform(-np.pi, np.pi)
        q[10], q[11] = np.cos(a), np.sin(a)
        q[12:16] = mdf.quat_axis_angle(mdf.random_unit(rg), rg.uniform(-1.0, 1.0))
        q[16] = rg.uniform(-2.5, 2.5)
        Rs = [frame_rotation(d, s, q) for s in range(n_imu)]
        ok, branches = True, []
        for R in Rs:
            br, dist = mdf.m2q_branch(R)
            branches.append(br)
            ok &= dist >= mdf.M2Q_MARGIN
        qe = np.full((4, n_imu), np.nan)
        ref["matrices_to_quat"](tuple(Rs), qe)
        if lane_kind == "regular":
            acc = f32(np.stack([mdf.random_unit(rg) * rg.uniform(5.0, 15.0) for _ in range(n_imu)], 1))
        else:
            acc = f32(rg.uniform(-low / 2, low / 2, size=(3, n_imu)))
            if lane_kind == "single":
                acc[int(rg.integers(3)), int(rg.integers(n_imu))] = f32(rg.choice([-1.0, 1.0]) * rg.uniform(2 * low, 12.0))
        # (every component away from the 0.1 g test by a factor 2)
        ok &= bool(((np.abs(acc) <= low / 2) | (np.abs(acc) >= 2 * low)).all())
        falling = bool((np.abs(acc) < low).all())
        ok &= falling == (lane_kind == "fallback")
        qa, names = qe.copy(), []
        if not falling:
            v = acc / np.linalg.norm(acc, axis=0)
            for s in range(n_imu):
                name, keeps = mdf.swing_branch(v[:, s])
                ok &= name == "regular" and bool(keeps) and v[2, s] >= VZ_MIN
                names.append(name)
            if ok:
                ref["swing_from_vector"]((v[0], v[1], v[2]), qa)
        re_, ra = np.empty((3, n_imu)), np.empty((3, n_imu))
        if ok:
            ref["quat_to_rpy"](qe, re_)
            ref["quat_to_rpy"](qa, ra)
            ok = rpy_ok(re_) and rpy_ok(ra)
        if not ok:
            rejected += 1
            if rejected > 400 * B:
                raise RuntimeError("too many rejected lanes")
            continue
        imu = np.concatenate([f32(rg.normal(size=(3, n_imu))), acc], 0).T
        q_all.append(q); imu_all.append(imu); exact.append(qe); acc_q.append(qa); rpy_e.append(re_); rpy_a.append(ra)
        kinds.append(lane_kind)
        for br in branches:
            m2q_hits[br] += 1
        for nm in names:
            swing_hits[nm] = swing_hits.get(nm, 0) + 1
    case = dict(d)
    case.update(n_imu=np.int32(n_imu), q=np.stack(q_all, -1), imu=np.stack(imu_all, -1), quat_exact=np.stack(exact, -1),
                quat_acc=np.stack(acc_q, -1), rpy_exact=np.stack(rpy_e, -1), rpy_acc=np.stack(rpy_a, -1),
                lane_kind=np.array(kinds), m2q_hits=m2q_hits, swing_hits=np.array(json.dumps(swing_hits, sort_keys=True)))
    return case, rejected


# ----------------------------------------------------------------------------------------------------------- body cases
def body_case(ref, rg, twist_time_constant, compute_rpy, dt=0.005):
    n_imu = 2
    rel = np.full((4, n_imu), np.nan)
    ref["matrices_to_quat"]((mdf.rot_rpy(0.4, -0.3, 1.2), mdf.rot_rpy(-1.1, 0.5, 2.6)), rel)
    remove = twist_time_constant is not None
    update = remove and twist_time_constant > 0.0
    tci = (1.0 / twist_time_constant) if update else (float("inf") if remove else 0.0)
    lanes, rejected = [], 0
    while len(lanes) < B:
        quat, omega, rpy, twist = np.zeros((4, n_imu)), np.zeros((3, n_imu)), np.zeros((3, n_imu)), np.zeros((1, n_imu))
        quat[3] = 1.0
        rec, ok = dict(imu_quat=[], imu_omega=[], quat=[], omega=[], twist=[], rpy=[]), True
        body = [upright_quat(rg, 0.8) for _ in range(n_imu)]
        for t in range(TICKS):
            # the body orientation drifts a little every tick; the IMU reads it turned by its mounting rotation
            body = [mdf.qmul(b, mdf.quat_axis_angle(mdf.random_unit(rg), rg.uniform(-0.05, 0.05))) for b in body]
            iq = np.stack([mdf.qmul(b, rel[:, s]) for s, b in enumerate(body)], 1)
            io = f32(rg.normal(scale=1.5, size=(3, n_imu)))
            ref["quat_multiply"](iq, rel, out=quat, is_right_conjugate=True)
            ref["quat_apply"](rel, io, out=omega)
            if remove:
                tilt = np.stack(ref["compute_tilt_from_quat"](quat))
                for s in range(n_imu):
                    name, keeps = mdf.swing_branch(tilt[:, s])
                    ok &= name == "regular" and bool(keeps) and tilt[2, s] >= VZ_MIN
                ref["remove_twist_from_quat"](quat)
            if update:
                ref["update_twist"](quat, twist, omega, tci, dt)
            ref["quat_to_rpy"](quat, rpy)
            ok &= rpy_ok(rpy) and bool(np.isfinite(quat).all())
            if not ok:
                break
            for k, v in dict(imu_quat=iq, imu_omega=io, quat=quat, omega=omega, twist=twist[0], rpy=rpy).items():
                rec[k].append(v.copy())
        if not ok:
            rejected += 1
            if rejected > 400 * B:
                raise RuntimeError("too many rejected lanes")
            continue
        lanes.append(rec)
    stack = lambda key: np.stack([np.stack(r[key]) for r in lanes], -1)     # noqa: E731
    case = dict(n_imu=np.int32(n_imu), rel_quat=rel.T.copy(), dt=np.float64(dt), twist_mode=np.int32(int(remove) + int(update)),
                time_constant_inv=np.float64(tci if update else 0.0), compute_rpy=np.int32(compute_rpy),
                imu_quat=stack("imu_quat"), imu_omega=stack("imu_omega"), quat=stack("quat"), omega=stack("omega"))
    if update:
        case["twist"] = stack("twist")
    if compute_rpy:
        case["rpy"] = stack("rpy")
    return case, rejected


def main(out_path: str) -> None:
    ref = load_reference_functions()
    rg = np.random.default_rng(SEED)
    out: dict = {}

    def put(group: str, label: str, got) -> None:
        case, rejected = got
        for k, v in case.items():
            out[f"{group}.{label}.{k}"] = v
        print(f"{group}.{label}: {rejected} lanes rejected" + (f", {case['hits']}" if "hits" in case else ""))

    mahony = []
    for n_imu in (1, 3):
        for ignore_twist in (0, 1):
            for compute_rpy in (0, 1):
                label = f"n{n_imu}_{'swing' if ignore_twist else 'twist'}_{'rpy' if compute_rpy else 'norpy'}"
                kinds = ("move",)
                if n_imu == 3 and not compute_rpy:
                    kinds = ("move", "rest")            # some lanes with every IMU at rest: the early return
                elif n_imu == 3:
                    kinds = ("move", "one")             # some lanes where exactly one of three IMUs moves
                put("mahony", label, mahony_case(ref, rg, n_imu, ignore_twist, compute_rpy, kinds))
                mahony.append(label)
    put("mahony", "n3_singular", mahony_case(ref, rg, 3, 1, 1, ("singular", "move"), dt=0.01, singular=True))
    mahony.append("n3_singular")
    out["mahony_cases"] = np.array(mahony)
    put("init", "joints", init_case(ref, rg))
    body = []
    for label, tau, compute_rpy in (("keep_rpy", None, 1), ("remove_norpy", 0.0, 0), ("leak_rpy", 0.5, 1), ("clamp_norpy", 0.002, 0)):
        put("body", label, body_case(ref, rg, tau, compute_rpy))
        body.append(label)
    out["body_cases"] = np.array(body)
    out["tier"] = np.array("A: the reference's functions on the arrays they are written for; the order of the calls, the "
                           "accelerometer test / normalisation and the frame rotations of the exact initialisation are restated")
    np.savez_compressed(out_path, **out)
    print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if not os.path.isdir(COMMON):
        sys.exit(f"{COMMON} not found: run this where the reference tree is available")
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
