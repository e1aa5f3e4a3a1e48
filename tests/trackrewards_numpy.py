"""The tracking rewards block in numpy (tests only): what `k_tracking_rewards` writes, and the error bounds its tests compare
against.  The names and layouts are those of tests/golden/ref_tracking_rewards.npz (tools/make_ref_tracking_rewards_fixtures.py).

plan: n_motors, n_frames, root_column, contact_column `[nc]`, and the same three of the reference side.  inputs, `[rows][B]`:
pose `[7][K][B]`, v_avg `[6][K][B]`, quat_no_yaw `[4][K][B]`, their `_reference` twins on K_ref columns, dcm / dcm_reference
`[2][B]`, position / position_reference `[M][B]`.  outputs: value, reference `[6 + M][B]`, rewards `[4][B]`.

The bounds.  E = eps of the kernel's dtype + eps of float64 (the expectation is a float64 result with a rounding of its own);
a float32 kernel reads its inputs rounded to float32, half an eps each, which the counts include.
  height          z_root - min z: the minimum is exact, the two roundings of the inputs and the subtraction: E (|z_root| + |z_min|)
  velocity        a row of `quat_apply` is sum_j c_j u_j with c_j a sum of four squares or of two doubled products of the
                  components of a unit quaternion, |c_j| <= 1: the roundings of the quaternion (2 eps on a product of two),
                  three sums (3 eps), the product with u_j and its rounding (1.5 eps), two sums of the row (2 eps): below
                  9 E sum_j |u_j|; 12 E |u|_1
  copies          capture point and joint positions: half an eps of the dtype where it is not float64's, else 0
  reward          r = CUTOFF_ESP^(s / c^2), s = sum e_i^2, e = value - reference with the bounds b_v, b_r above:
                  de_i = b_v + b_r + E |e_i|; ds = sum (2 |e_i| de_i + de_i^2 + 2 E e_i^2); x = s / c^2: dx = ds / c^2 + 3 E x
                  (the square of the cutoff, the division); r = exp(x ln CUTOFF_ESP): dr = r (|ln CUTOFF_ESP| dx + 8 E), the
                  8 E for a `pow` good to 4 ulp on either side.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tracking_rewards.npz")
PLAN_KEYS = ("n_motors", "n_frames", "root_column", "contact_column", "n_frames_reference", "root_column_reference",
             "contact_column_reference")
INPUTS = ("pose", "pose_reference", "v_avg", "quat_no_yaw", "v_avg_reference", "quat_no_yaw_reference", "dcm", "dcm_reference",
          "position", "position_reference")
OUTPUTS = ("value", "reference", "rewards")
TERMS = ("base_height", "odometry_velocity", "capture_point", "joint_positions")
CUTOFF_ESP = 1.0e-2
FIXED_ROWS = 6
TERM_ROWS = {0: slice(0, 1), 1: slice(1, 4), 2: slice(4, 6), 3: slice(6, None)}


def load_cases() -> Dict[str, dict]:
    z = np.load(GOLDEN)
    cases: Dict[str, dict] = {}
    for name in z["cases"]:
        prefix = f"{name}."
        cases[str(name)] = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}
    return cases


def plan_of(case: dict) -> dict:
    plan = {k[5:]: v for k, v in case.items() if k.startswith("plan.")}
    return {k: (v if v.ndim else v.item()) for k, v in plan.items()}


def rows_of(name: str, plan: dict) -> int:
    return 4 if name == "rewards" else FIXED_ROWS + int(plan["n_motors"])


def quat_apply(q: np.ndarray, u: np.ndarray) -> np.ndarray:
    """Rotation of `u` `[3][...]` by the unit quaternions `q` `[4][...]` (xyzw)."""
    x, y, z, w = q
    return np.stack([u[0] * (x * x + w * w - y * y - z * z) + u[1] * (2 * x * y - 2 * z * w) + u[2] * (2 * x * z + 2 * y * w),
                     u[0] * (2 * z * w + 2 * x * y) + u[1] * (w * w - x * x + y * y - z * z) + u[2] * (-2 * x * w + 2 * y * z),
                     u[0] * (-2 * y * w + 2 * x * z) + u[1] * (2 * x * w + 2 * y * z) + u[2] * (w * w - x * x - y * y + z * z)])


def run(plan: dict, inputs: Dict[str, np.ndarray], cutoff: Sequence[Optional[float]], dtype=np.float64) -> Dict[str, np.ndarray]:
    """The block on every lane in float64: `value`, `reference`, `rewards` and `bound.<output>` for a kernel of `dtype`.  A
    term whose cutoff is None or whose inputs are missing is skipped: its rows are zero with a zero bound."""
    B = next(iter(inputs.values())).shape[-1]
    eps_t = float(np.finfo(np.dtype(dtype)).eps)
    E = eps_t + float(np.finfo(np.float64).eps)
    copy = 0.0 if np.dtype(dtype) == np.float64 else 0.5 * eps_t
    rows = rows_of("value", plan)
    out = {k: np.zeros((rows, B)) for k in ("value", "reference", "bound.value", "bound.reference")}
    out["rewards"], out["bound.rewards"] = np.zeros((4, B)), np.zeros((4, B))
    has = lambda *names: all(n in inputs for n in names)      # noqa: E731
    sides = (("value", "", ""), ("reference", "_reference", "_reference"))
    done = []
    if cutoff[0] is not None and has("pose", "pose_reference"):
        for key, suffix, _ in sides:
            z = inputs["pose" + suffix][2]
            root, lowest = z[int(plan["root_column" + suffix])], z[np.asarray(plan["contact_column" + suffix])].min(axis=0)
            out[key][0], out["bound." + key][0] = root - lowest, E * (np.abs(root) + np.abs(lowest))
        done.append(0)
    if cutoff[1] is not None and has("v_avg", "quat_no_yaw", "v_avg_reference", "quat_no_yaw_reference"):
        for key, suffix, _ in sides:
            root = int(plan["root_column" + suffix])
            v, q = inputs["v_avg" + suffix][:, root], inputs["quat_no_yaw" + suffix][:, root]
            lin, ang = quat_apply(q, v[:3]), quat_apply(q, v[3:])
            out[key][1:4] = np.stack([lin[0], lin[1], ang[2]])
            l1, a1 = np.abs(v[:3]).sum(axis=0), np.abs(v[3:]).sum(axis=0)
            out["bound." + key][1:4] = 12 * E * np.stack([l1, l1, a1])
        done.append(1)
    if cutoff[2] is not None and has("dcm", "dcm_reference"):
        for key, suffix, _ in sides:
            out[key][4:6], out["bound." + key][4:6] = inputs["dcm" + suffix], copy * np.abs(inputs["dcm" + suffix])
        done.append(2)
    if cutoff[3] is not None and has("position", "position_reference") and int(plan["n_motors"]) > 0:
        for key, suffix, _ in sides:
            out[key][6:], out["bound." + key][6:] = inputs["position" + suffix], copy * np.abs(inputs["position" + suffix])
        done.append(3)
    for term in done:
        r = TERM_ROWS[term]
        e = out["value"][r] - out["reference"][r]
        de = out["bound.value"][r] + out["bound.reference"][r] + E * np.abs(e)
        s, ds = np.sum(e * e, axis=0), np.sum(2 * np.abs(e) * de + de * de + 2 * E * e * e, axis=0)
        c2 = float(cutoff[term]) ** 2
        x, dx = s / c2, ds / c2 + 3 * E * s / c2
        reward = np.power(CUTOFF_ESP, x)
        out["rewards"][term], out["bound.rewards"][term] = reward, reward * (abs(np.log(CUTOFF_ESP)) * dx + 8 * E)
    return out


def compare(name: str, got: np.ndarray, expected: np.ndarray, bound: np.ndarray) -> float:
    """Assert `got` against `expected`: bit for bit where `bound` is 0, inside the bound elsewhere.  Returns the worst error over
    its bound."""
    got, expected = np.asarray(got), np.asarray(expected)
    assert got.shape == expected.shape == bound.shape, (name, got.shape, expected.shape, bound.shape)
    exact = bound == 0
    assert np.array_equal(got[exact].astype(np.float64), expected[exact]), f"{name}: the exact entries differ"
    if not (~exact).any():
        return 0.0
    ratio = np.abs(got.astype(np.float64) - expected)[~exact] / bound[~exact]
    worst = float(ratio.max())
    assert worst <= 1.0, f"{name}: worst error over its bound {worst:.3g}"
    return worst
