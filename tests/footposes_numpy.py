"""An authored numpy statement of what the foot pose quantities block computes (tests only), vectorised over the lanes in the
arithmetic of a given dtype (float64, float32): a second statement next to the reference's own output
(tests/golden/ref_footposes.npz) and the yardstick of the float32 tolerance.  The quaternion average of three feet or more is
`np.linalg.eigh` in that dtype, with the block's sign (a non-negative dot product with the first foot's quaternion).

`plan`: foot_column, n_frames, position_cutoff, orientation_cutoff.  `inputs`: pose `[7][K][B]`, reference_relative_pose
`[7][F-1][B]` (optional).
"""
from __future__ import annotations

from typing import Dict

import numpy as np

CUTOFF_ESP = 1.0e-2
INPUTS = ("pose", "reference_relative_pose")
OUTPUTS = ("mean_pose", "mean_odom_pose", "relative_pose", "tracking_error", "scalars")
# the outputs downstream of the eigenvector (three feet or more): everything but the mean position
EIGEN_OUTPUTS = ("mean_pose", "mean_odom_pose", "relative_pose", "tracking_error", "scalars")


def output_shape(name: str, plan: Dict, B: int) -> tuple:
    R = len(plan["foot_column"]) - 1
    return {"mean_pose": (7, B), "mean_odom_pose": (3, B), "relative_pose": (7, R, B), "tracking_error": (6, R, B), "scalars": (2, B)}[name]


def load_case(npz, label: str):
    """`plan`, `inputs`, `expected` of one case of tests/golden/ref_footposes.npz."""
    pre = label + "."
    keys = [k[len(pre):] for k in npz.files if k.startswith(pre)]
    plan = {k[5:]: npz[pre + k] for k in keys if k.startswith("plan.")}
    plan = {k: (v if v.ndim else v.item()) for k, v in plan.items()}
    inputs = {k: npz[pre + k] for k in keys if k in INPUTS}
    expected = {k[9:]: npz[pre + k] for k in keys if k.startswith("expected.")}
    return plan, inputs, expected


def quat_mul_conj_left(l, r):
    """`quat_multiply(l, r, is_left_conjugate=True)` (utils/math.py:611-622: the sign goes to w of the left factor, which
    gives minus the Hamilton product conj(l) r -- the same rotation), quaternions xyzw `[4][...]`."""
    lx, ly, lz, lw = l
    rx, ry, rz, rw = r
    return np.stack([-lw * rx + lx * rw + ly * rz - lz * ry, -lw * ry - lx * rz + ly * rw + lz * rx,
                     -lw * rz + lx * ry - ly * rx + lz * rw, -lw * rw - lx * rx - ly * ry - lz * rz])


def quat_matrix(q):
    """Rotation matrices `[3][3][...]` of quaternions xyzw `[4][...]`."""
    x, y, z, w = q
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)]),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)]),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)])])


def log3(q, dtype):
    vec, w = q[:3], q[3]
    theta_sin_2 = np.sqrt(np.sum(np.square(vec), 0))
    theta = 2 * np.arctan2(theta_sin_2, np.abs(w))
    return theta / np.maximum(theta_sin_2, np.finfo(dtype).tiny) * vec * np.sign(w)


def gram(quats: np.ndarray) -> np.ndarray:
    """sum over the feet of q q^T, `[B][4][4]`, of quaternions `[4][F][B]`."""
    return np.einsum("ifb,jfb->bij", quats, quats)


def mean_quaternion(quats: np.ndarray, dtype) -> np.ndarray:
    """`quat_average_2d` per lane: quaternions `[4][F][B]` -> `[4][B]`."""
    F = quats.shape[1]
    if F == 1:
        return quats[:, 0].copy()
    if F == 2:
        q1, q2 = quats[:, 0], quats[:, 1]
        dot = np.sum(q1 * q2, 0)
        return (q1 + np.sign(dot) * q2) / np.sqrt(2 * (1 + np.abs(dot)))
    M = np.zeros((quats.shape[2], 4, 4), dtype=dtype)
    for f in range(F):
        M = M + quats[:, f].T[:, :, None] * quats[:, f].T[:, None, :]
    mean = np.linalg.eigh(M)[1][:, :, -1].T.astype(dtype)
    return mean * np.where(np.sum(mean * quats[:, 0], 0) < 0, dtype(-1), dtype(1))


def quantities(plan: Dict, inputs: Dict, dtype=np.float64) -> Dict[str, np.ndarray]:
    dtype = np.dtype(dtype).type
    pose = np.asarray(inputs["pose"], dtype=dtype)[:, [int(c) for c in plan["foot_column"]]]
    F, B = pose.shape[1:]
    positions, quats = pose[:3], pose[3:]
    total = positions[:, 0].copy()
    for f in range(1, F):
        total = total + positions[:, f]
    p_mean = total / dtype(F)
    q_mean = mean_quaternion(quats, dtype)
    x, y, z, w = q_mean
    yaw = np.arctan2(2 * (y * x + z * w), 1 - 2 * (y * y + z * z))
    out = {"mean_pose": np.concatenate([p_mean, q_mean]), "mean_odom_pose": np.stack([p_mean[0], p_mean[1], yaw])}
    R = quat_matrix(q_mean)                                    # [3][3][B]
    d = positions[:, :-1] - p_mean[:, None, :]                 # [3][F-1][B]
    rel_p = np.stack([R[0, i][None] * d[0] + R[1, i][None] * d[1] + R[2, i][None] * d[2] for i in range(3)])
    rel_q = quat_mul_conj_left(q_mean[:, None, :], quats[:, :-1])
    out["relative_pose"] = np.concatenate([rel_p, rel_q]).astype(dtype)
    ref = inputs.get("reference_relative_pose")
    if ref is not None or F == 1:
        ref = np.zeros((7, 0, B), dtype=dtype) if ref is None else np.asarray(ref, dtype=dtype)
        e_p = rel_p - ref[:3]
        e_q = log3(quat_mul_conj_left(rel_q, ref[3:]), dtype)
        out["tracking_error"] = np.concatenate([e_p, e_q]).astype(dtype)
        rbf = lambda e, cutoff: np.power(dtype(CUTOFF_ESP), np.sum(e * e, (0, 1), dtype=dtype) / np.power(dtype(cutoff), dtype(2)))  # noqa: E731
        out["scalars"] = np.stack([rbf(e_p, plan["position_cutoff"]), rbf(e_q, plan["orientation_cutoff"])])
    assert all(v.dtype == dtype for v in out.values()), {k: v.dtype for k, v in out.items()}
    return out


def align_sign(got: Dict[str, np.ndarray], want: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The comparison rule for three feet or more: per lane, the mean and every relative quaternion of `got` times the sign
    of the dot product of its mean quaternion with that of `want`."""
    s = np.where(np.sum(got["mean_pose"][3:].astype(np.float64) * want["mean_pose"][3:], 0) < 0, -1.0, 1.0)
    out = {k: v.copy() for k, v in got.items()}
    out["mean_pose"][3:] *= s.astype(got["mean_pose"].dtype)
    if "relative_pose" in out:
        out["relative_pose"][3:] *= s.astype(got["relative_pose"].dtype)
    return out
