"""An authored numpy statement of what the tracking windows block computes (tests only), vectorised over the lanes in the
arithmetic of a given dtype (float64, float32): a second statement next to the reference's own output
(tests/golden/ref_tracking.npz), the expected value of the float32 tests and the home of the derived error bounds.

`plan`: max_stack_odom, max_stack_foot, max_stack_motor (0: the family is absent), n_rel, n_motors, and the launch scalar of a
fixture case, odometry_cutoff.  `inputs`: odom_pose, reference_odom_pose `[3][B]`, relative_pose, reference_relative_pose
`[7][R][B]`, position, reference_position `[M][B]`; the inputs of an absent family are missing.

A fixture case is a sequence of launches ("events"): `mode [E]` (0 restart, 1 push), `mask [E][B]`, every input per event
(`[E]` in front), and under `expected.` the tensors and the state of the block after every event -- a lane that an event's mask
leaves out keeps what it had.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

CUTOFF_ESP = 1.0e-2
RESTART, PUSH = 0, 1
DRIFT_POSITION, DRIFT_ORIENTATION, REWARD_ODOM_POSE, SHIFT_FOOT_POSITIONS, SHIFT_FOOT_ORIENTATIONS, SHIFT_MOTOR_POSITIONS = range(6)
FAMILY_INPUTS = {"odom": ("odom_pose", "reference_odom_pose"), "foot": ("relative_pose", "reference_relative_pose"),
                 "motor": ("position", "reference_position")}
FAMILY_STATE = {"odom": ("odom_ring", "yaw_prev", "yaw_ring"), "foot": ("foot_ring",), "motor": ("motor_ring",)}
FAMILY_ROWS = {"odom": (DRIFT_POSITION, DRIFT_ORIENTATION, REWARD_ODOM_POSE), "foot": (SHIFT_FOOT_POSITIONS, SHIFT_FOOT_ORIENTATIONS),
               "motor": (SHIFT_MOTOR_POSITIONS,)}
INPUTS = tuple(n for names in FAMILY_INPUTS.values() for n in names)
STATE = ("count",) + tuple(n for names in FAMILY_STATE.values() for n in names)
OUTPUTS = ("delta_odom", "delta_odom_reference", "scalars")
PLAN_KEYS = ("max_stack_odom", "max_stack_foot", "max_stack_motor", "n_rel", "n_motors")
# the error of the device's atan2 in units in the last place of its result.  tests/device_math pins no atan2 of its own (it pins
# `quat_log3`, which ends in one, to its contract); the figure is the limit the device library documents for the function,
# which is OpenCL's: 6 ulp.  numpy's (the C library's) is below 1 ulp and inside the margin.
ATAN2_ULP = 6.0


def families(plan: Dict):
    return [f for f in ("odom", "foot", "motor") if int(plan[f"max_stack_{f}"]) > 0]


def state_names(plan: Dict):
    return ("count",) + tuple(n for f in families(plan) for n in FAMILY_STATE[f])


def shape(name: str, plan: Dict, B: int) -> tuple:
    So, Sf, Sm, R, M = (int(plan[k]) for k in PLAN_KEYS)
    return {"odom_pose": (3, B), "reference_odom_pose": (3, B), "relative_pose": (7, R, B), "reference_relative_pose": (7, R, B),
            "position": (M, B), "reference_position": (M, B), "count": (B,), "odom_ring": (So, 4, B), "yaw_prev": (2, B),
            "yaw_ring": (So - 1, 2, B), "foot_ring": (2, Sf, B), "motor_ring": (Sm, B), "delta_odom": (3, B),
            "delta_odom_reference": (3, B), "scalars": (6, B)}[name]


def dtype_of(name: str, dtype):
    return np.dtype(np.int32) if name == "count" else np.dtype(dtype)


def load_case(npz, label: str):
    """`plan`, the inputs, `mode [E]`, `mask [E][B]` and `expected` of one case of tests/golden/ref_tracking.npz."""
    pre = label + "."
    own = {k[len(pre):]: npz[k] for k in npz.files if k.startswith(pre)}
    plan = {k[5:]: v.item() for k, v in own.items() if k.startswith("plan.")}
    inputs = {k: own[k] for k in INPUTS if k in own}
    expected = {k[9:]: v for k, v in own.items() if k.startswith("expected.")}
    return plan, inputs, own["mode"], own["mask"], expected


def event_inputs(inputs: Dict, e: int) -> Dict:
    return {k: v[e] for k, v in inputs.items()}


def new_state(plan: Dict, B: int, dtype=np.float64) -> Dict[str, np.ndarray]:
    return {n: np.zeros(shape(n, plan, B), dtype=dtype_of(n, dtype)) for n in state_names(plan)}


def angle_difference(left, right, pi):
    delta = left - right
    return delta - np.floor((delta + pi) / (2 * pi)) * (2 * pi)


def angle_distance(left, right, pi):
    delta = left - right
    delta = delta - np.floor(delta / (2 * pi)) * (2 * pi)
    return pi - np.abs(delta - pi)


def pose_yaw(pose):
    x, y, z, w = pose[3], pose[4], pose[5], pose[6]
    return np.arctan2(2 * (y * x + z * w), 1 - 2 * (y * y + z * z))


def foot_squares(inputs: Dict, dtype=np.float64):
    """`[2][B]`: the two sums of squares of one timestamp, in the row order of `min_norm`."""
    dtype = np.dtype(dtype).type
    rel, ref = np.asarray(inputs["relative_pose"], dtype=dtype), np.asarray(inputs["reference_relative_pose"], dtype=dtype)
    B = rel.shape[-1]
    sq_p, sq_o = np.zeros(B, dtype=dtype), np.zeros(B, dtype=dtype)
    for c in range(2):
        for j in range(rel.shape[1]):
            e = rel[c, j] - ref[c, j]
            sq_p = sq_p + e * e
    with np.errstate(invalid="ignore"):
        dist = angle_distance(pose_yaw(rel), pose_yaw(ref), dtype(np.pi))
    for j in range(rel.shape[1]):
        sq_o = sq_o + dist[j] * dist[j]
    return np.stack([sq_p, sq_o])


def motor_squares(inputs: Dict, dtype=np.float64):
    dtype = np.dtype(dtype).type
    e = np.asarray(inputs["position"], dtype=dtype) - np.asarray(inputs["reference_position"], dtype=dtype)
    sq = np.zeros(e.shape[-1], dtype=dtype)
    for m in range(e.shape[0]):
        sq = sq + e[m] * e[m]
    return sq


def _push_min(ring, S, count, value, lanes):
    """`value [B]` into slot count % S of `ring [S][B]` on `lanes`; the NaN-propagating minimum of the slots in use."""
    ring[(count % S)[lanes], lanes] = value[lanes]
    n = np.minimum(count + 1, S)
    use = np.arange(S)[:, None] < n[None, :]
    with np.errstate(invalid="ignore"):
        return np.where(use, ring, np.inf).min(0)       # (np.min propagates NaN; slot 0 is always in use)


def quantities(plan: Dict, inputs: Dict, state: Dict[str, np.ndarray], mode: int, mask: Optional[np.ndarray] = None,
               dtype=np.float64, odometry_cutoff=None) -> Dict[str, np.ndarray]:
    """One launch.  Returns every output for every lane; `state` is updated in place on the lanes of `mask` (all without
    one), and the outputs are meaningful on those lanes only.  Rows of absent families stay zero."""
    dtype = np.dtype(dtype).type
    cutoff = dtype(plan["odometry_cutoff"] if odometry_cutoff is None else odometry_cutoff)
    B = state["count"].shape[0]
    mask = np.ones(B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    lanes = np.flatnonzero(mask)
    count = state["count"]
    count[lanes] = 0 if mode == RESTART else count[lanes] + 1
    out = {k: np.zeros(shape(k, plan, B), dtype=dtype) for k in OUTPUTS}
    scalars = out["scalars"]
    pi = dtype(np.pi)
    with np.errstate(invalid="ignore"):
        if "odom" in families(plan):
            S = int(plan["max_stack_odom"])
            ring, yaw_prev, yaw_ring = state["odom_ring"], state["yaw_prev"], state["yaw_ring"]
            slot, oldest = count % S, np.where(count + 1 >= S, (count + 1) % S, 0)
            yaw_slot, yaw_n = count % (S - 1), np.minimum(count + 1, S - 1)
            for s, (name, key) in enumerate((("odom_pose", "delta_odom"), ("reference_odom_pose", "delta_odom_reference"))):
                pose = np.asarray(inputs[name], dtype=dtype)
                ring[slot[lanes], 2 * s, lanes], ring[slot[lanes], 2 * s + 1, lanes] = pose[0, lanes], pose[1, lanes]
                every = np.arange(B)
                out[key][0], out[key][1] = pose[0] - ring[oldest, 2 * s, every], pose[1] - ring[oldest, 2 * s + 1, every]
                previous = pose[2] if mode == RESTART else yaw_prev[s]
                step = angle_difference(pose[2], previous, pi)
                yaw_prev[s, lanes] = pose[2, lanes]
                yaw_ring[yaw_slot[lanes], s, lanes] = step[lanes]
                total = np.zeros(B, dtype=dtype)
                for k in range(S - 1):       # (storage order)
                    total = np.where(k < yaw_n, total + yaw_ring[k, s], total)
                out[key][2] = total
            dt, dr = out["delta_odom"], out["delta_odom_reference"]
            ex, ey, eyaw = dt[0] - dr[0], dt[1] - dr[1], dt[2] - dr[2]
            scalars[DRIFT_POSITION], scalars[DRIFT_ORIENTATION] = np.sqrt(ex * ex + ey * ey), np.abs(eyaw)
            if cutoff > 0:
                en = np.sqrt(dt[0] * dt[0] + dt[1] * dt[1]) - np.sqrt(dr[0] * dr[0] + dr[1] * dr[1])
                scalars[REWARD_ODOM_POSE] = np.power(dtype(CUTOFF_ESP), (en * en + eyaw * eyaw) / np.power(cutoff, dtype(2)))
        if "foot" in families(plan):
            S = int(plan["max_stack_foot"])
            sq = foot_squares(inputs, dtype)
            scalars[SHIFT_FOOT_POSITIONS] = np.sqrt(_push_min(state["foot_ring"][0], S, count, sq[0], lanes))
            scalars[SHIFT_FOOT_ORIENTATIONS] = np.sqrt(_push_min(state["foot_ring"][1], S, count, sq[1], lanes))
        if "motor" in families(plan):
            S = int(plan["max_stack_motor"])
            scalars[SHIFT_MOTOR_POSITIONS] = np.sqrt(_push_min(state["motor_ring"], S, count, motor_squares(inputs, dtype), lanes))
    assert all(v.dtype == dtype for v in out.values())
    return out


def replay(plan: Dict, inputs: Dict, modes, masks, dtype=np.float64, step=None):
    """Every event of a case through `step(inputs of the event, state, mode, mask) -> outputs` (default: `quantities`), with
    the carry-over of the lanes an event leaves out.  Returns `[E]`-stacked outputs and states like the fixture's `expected`."""
    B = np.asarray(masks).shape[-1]
    state = new_state(plan, B, dtype)
    if step is None:
        step = lambda inp, st, mode, mask: quantities(plan, inp, st, mode, mask, dtype)      # noqa: E731
    held, rows = None, []
    for e, (mode, mask) in enumerate(zip(modes, masks)):
        mask = np.asarray(mask, dtype=bool)
        got = step(event_inputs(inputs, e), state, int(mode), mask)
        if held is None:
            assert np.all(mask), "the first event of a case launches every lane"
            held = {k: np.array(v) for k, v in got.items()}
        else:
            for k, v in got.items():
                held[k][..., mask] = v[..., mask]
        rows.append({**{k: v.copy() for k, v in held.items()}, **{k: v.copy() for k, v in state.items()}})
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


# ---------------------------------------------------------------------------------------------------- the derived bounds
# Every bound is on |got - want| where `want` is the float64 value of the reference and `got` is computed in arithmetic of unit
# `eps` from the same inputs (the fixture's inputs are exact in float32).  Each counts the roundings of both sides, with a
# factor 2 of margin inside the constants; NaN lanes are compared as patterns, not through a bound.
def _step_bound(yaw, previous, eps):
    """`angle_difference`: the subtraction, the product k 2 pi with the rounded constant (|k| <= 1: 2 pi eps each for the
    constant and the product), the final subtraction.  The floor is exact: its argument stays away from an integer."""
    raw = yaw - previous
    k = np.floor((raw + np.pi) / (2 * np.pi))
    return 2.0 * eps * (np.abs(raw) + 4.0 * np.pi * np.abs(k) + np.abs(raw - k * 2 * np.pi))


def _yaw_bound(pose, eps):
    """The error of `quat_to_yaw`: the roundings of sin = 2 (xy + zw) and cos = 1 - 2 (yy + zz) turned into an angle
    (divided by the length of (sin, cos)), plus ATAN2_ULP units of the result."""
    x, y, z, w = pose[3], pose[4], pose[5], pose[6]
    sn, cs = 2 * (y * x + z * w), 1 - 2 * (y * y + z * z)
    d_sn = 4.0 * eps * (np.abs(y * x) + np.abs(z * w))
    d_cs = 2.0 * eps * (1.0 + 2.0 * (y * y + z * z)) + 4.0 * eps * (y * y + z * z)
    return (d_sn + d_cs) / np.hypot(sn, cs) + (ATAN2_ULP + 1.0) * eps * np.abs(np.arctan2(sn, cs))


def _square_sum_bound(e, be, eps):
    """sum_i e_i^2 of `e [N][B]` with per-entry bounds `be`: 2 |e| be per entry, and (N + 3) eps of the sum on either side."""
    return (2.0 * np.abs(e) * be + be * be).sum(0) + 2.0 * (e.shape[0] + 3) * eps * (e * e).sum(0)


def foot_square_bounds(inputs: Dict, eps: float) -> np.ndarray:
    """`[2][B]`: the bounds of the two sums of squares of one timestamp."""
    rel, ref = np.asarray(inputs["relative_pose"], dtype=np.float64), np.asarray(inputs["reference_relative_pose"], dtype=np.float64)
    e = (rel[:2] - ref[:2]).reshape(-1, rel.shape[-1])
    position = _square_sum_bound(e, eps * np.abs(e), eps)
    with np.errstate(invalid="ignore"):
        yt, yr = pose_yaw(rel), pose_yaw(ref)
        dist = angle_distance(yt, yr, np.pi)
        # `angle_distance`: the two yaws, their difference, k 2 pi (|k| <= 1), pi - |delta - pi|: 4 roundings of at most 2 pi
        b_dist = _yaw_bound(rel, eps) + _yaw_bound(ref, eps) + 2.0 * eps * (np.abs(yt - yr) + 4.0 * np.pi + 2.0 * np.pi)
        orientation = _square_sum_bound(dist, b_dist, eps)
    return np.stack([position, orientation])


def motor_square_bound(inputs: Dict, eps: float) -> np.ndarray:
    e = np.asarray(inputs["position"], dtype=np.float64) - np.asarray(inputs["reference_position"], dtype=np.float64)
    return _square_sum_bound(e, eps * np.abs(e), eps)


def _sqrt_bound(value, bound, eps):
    """sqrt(v) with |dv| <= bound: dv / (sqrt(v) + sqrt(max(v - dv, 0))) <= min(dv / sqrt(v), sqrt(dv)), plus its rounding."""
    with np.errstate(invalid="ignore", divide="ignore"):
        root = np.sqrt(value)
        return np.minimum(np.where(root > 0, bound / root, np.inf), np.sqrt(bound)) + 2.0 * eps * root


def _min_bound(ring_v, ring_b, n):
    """The minimum over the slots in use moves by at most the largest bound of a slot in use."""
    use = np.arange(ring_v.shape[0])[:, None] < n[None, :]
    return np.where(use, ring_b, 0.0).max(0)


def bounds(plan: Dict, inputs: Dict, modes, masks, expected: Dict, eps: float) -> Dict[str, np.ndarray]:
    """The bounds of `delta_odom`, `delta_odom_reference`, `scalars` and of the rings that hold computed values (`yaw_ring`,
    `foot_ring`, `motor_ring`) after every event of a case, `[E]` in front, from float64 values.  `odom_ring`, `yaw_prev` and
    `count` hold copies and integers: they are exact."""
    B = np.asarray(masks).shape[-1]
    fam = families(plan)
    So, Sf, Sm = (int(plan[f"max_stack_{f}"]) for f in ("odom", "foot", "motor"))
    count = np.zeros(B, dtype=int)
    st = new_state(plan, B)                             # the float64 values of the rings
    sb = {n: np.zeros_like(st[n]) for n in ("yaw_ring", "foot_ring", "motor_ring") if n in st}
    held = {k: np.zeros(shape(k, plan, B)) for k in OUTPUTS}
    cutoff = float(plan["odometry_cutoff"])
    rows = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for e, (mode, mask) in enumerate(zip(modes, masks)):
            mask = np.asarray(mask, dtype=bool)
            lanes = np.flatnonzero(mask)
            inp = event_inputs(inputs, e)
            previous = {s: st["yaw_prev"][s].copy() for s in range(2)} if "odom" in fam else None
            want = quantities(plan, inp, st, int(mode), mask, np.float64)        # (updates `st`)
            count[lanes] = 0 if int(mode) == RESTART else count[lanes] + 1
            now = {k: np.zeros_like(v) for k, v in held.items()}
            if "odom" in fam:
                n = np.minimum(count + 1, So - 1)
                use = np.arange(So - 1)[:, None] < n[None, :]
                for s, (name, key) in enumerate((("odom_pose", "delta_odom"), ("reference_odom_pose", "delta_odom_reference"))):
                    pose = np.asarray(inp[name], dtype=np.float64)
                    prev = pose[2] if int(mode) == RESTART else previous[s]
                    sb["yaw_ring"][(count % (So - 1))[lanes], s, lanes] = _step_bound(pose[2], prev, eps)[lanes]
                    now[key][:2] = eps * np.abs(want[key][:2])
                    now[key][2] = np.where(use, sb["yaw_ring"][:, s], 0.0).sum(0) + \
                        2.0 * n * eps * np.where(use, np.abs(st["yaw_ring"][:, s]), 0.0).sum(0)
                dt, dr, bt, br = want["delta_odom"], want["delta_odom_reference"], now["delta_odom"], now["delta_odom_reference"]
                err, b_err = dt - dr, bt + br + eps * np.abs(dt - dr)
                norm = np.hypot(err[0], err[1])
                now["scalars"][DRIFT_POSITION] = b_err[0] + b_err[1] + 4.0 * eps * norm
                now["scalars"][DRIFT_ORIENTATION] = b_err[2]
                if cutoff > 0:
                    nt, nr = np.hypot(dt[0], dt[1]), np.hypot(dr[0], dr[1])
                    en = nt - nr
                    b_en = bt[0] + bt[1] + br[0] + br[1] + 4.0 * eps * (nt + nr) + eps * np.abs(en)
                    sq = en * en + err[2] * err[2]
                    b_sq = 2.0 * np.abs(en) * b_en + b_en ** 2 + 2.0 * np.abs(err[2]) * b_err[2] + b_err[2] ** 2 + 6.0 * eps * sq
                    # r = 0.01^(sq / cutoff^2): r ln(100) (b_sq / cutoff^2 + 4 eps sq / cutoff^2) + 8 eps (as the siblings' reward rows)
                    r = expected["scalars"][e][REWARD_ODOM_POSE]
                    now["scalars"][REWARD_ODOM_POSE] = r * np.log(100.0) * (b_sq + 4.0 * eps * sq) / cutoff ** 2 + 8.0 * eps
            if "foot" in fam:
                sb["foot_ring"][:, (count % Sf)[lanes], lanes] = foot_square_bounds(inp, eps)[:, lanes]
                n = np.minimum(count + 1, Sf)
                for row, k in ((SHIFT_FOOT_POSITIONS, 0), (SHIFT_FOOT_ORIENTATIONS, 1)):
                    now["scalars"][row] = _sqrt_bound(want["scalars"][row] ** 2, _min_bound(st["foot_ring"][k], sb["foot_ring"][k], n), eps)
            if "motor" in fam:
                sb["motor_ring"][(count % Sm)[lanes], lanes] = motor_square_bound(inp, eps)[lanes]
                n = np.minimum(count + 1, Sm)
                now["scalars"][SHIFT_MOTOR_POSITIONS] = _sqrt_bound(want["scalars"][SHIFT_MOTOR_POSITIONS] ** 2,
                                                                    _min_bound(st["motor_ring"], sb["motor_ring"], n), eps)
            for k in held:
                held[k][..., mask] = now[k][..., mask]
            rows.append({**{k: v.copy() for k, v in held.items()}, **{k: v.copy() for k, v in sb.items()}})
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}
