"""Independent numpy statements of what the frame kinematics block computes (tests only).

* Forward kinematics over a `CompiledModel` in float64 with 4x4 homogeneous transforms per joint, and the frame velocity
  from the columns of the geometric Jacobian (`[z x (p - p_j); z]` for a rotation about the world axis z through p_j,
  `[z; 0]` for a translation along z).  This is not the recursion of the kernel, which carries a rotation, a position and
  two velocity vectors along one walk per frame.
* The SE3 step average, restated from the reference's utils/math.py in the arithmetic of a given dtype (float64, float32):
  the yardstick of the float32 tolerance and a second statement next to the reference's own output (tests/golden/ref_frames.npz).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from jiminy_amd.attitude import matrix_to_quat
from jiminy_amd.model import (JT_FREEFLYER, JT_PU, JT_PX, JT_PZ, JT_RU, JT_RUBU, JT_RUBX, JT_RUBZ, JT_RX, JT_RZ, JT_SPHERICAL,
                              CompiledModel)

LOCAL, LOCAL_WORLD_ALIGNED, ODOMETRY = 0, 1, 2


# ------------------------------------------------------------------------------------------------- forward kinematics
def _hom(R: np.ndarray, p: np.ndarray) -> np.ndarray:
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, p
    return M


def _skew(a: np.ndarray) -> np.ndarray:
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def _rot(axis: np.ndarray, c: float, s: float) -> np.ndarray:
    K = _skew(axis)
    return np.eye(3) + s * K + (1.0 - c) * (K @ K)


def _quat_matrix(q: np.ndarray) -> np.ndarray:
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _axis(model: CompiledModel, j: int) -> np.ndarray:
    t = int(model.jtypes[j])
    for first, last, general in ((JT_RX, JT_RZ, JT_RU), (JT_PX, JT_PZ, JT_PU), (JT_RUBX, JT_RUBZ, JT_RUBU)):
        if first <= t <= last:
            return np.eye(3)[t - first]
        if t == general:
            return np.asarray(model.axes[j], dtype=np.float64)
    raise AssertionError(t)


def joint_motion(model: CompiledModel, j: int, q: np.ndarray) -> np.ndarray:
    """4x4 transform of the motion of joint j at configuration `q` (one lane)."""
    t, iq = int(model.jtypes[j]), int(model.idx_q[j])
    if t == JT_FREEFLYER:
        return _hom(_quat_matrix(q[iq + 3:iq + 7]), q[iq:iq + 3])
    if t == JT_SPHERICAL:
        return _hom(_quat_matrix(q[iq:iq + 4]), np.zeros(3))
    a = _axis(model, j)
    if JT_PX <= t <= JT_PU:
        return _hom(np.eye(3), a * q[iq])
    if JT_RUBX <= t <= JT_RUBU:
        return _hom(_rot(a, q[iq], q[iq + 1]), np.zeros(3))
    return _hom(_rot(a, np.cos(q[iq]), np.sin(q[iq])), np.zeros(3))


def joint_transforms(model: CompiledModel, q: np.ndarray, placement_p: Optional[np.ndarray] = None) -> list:
    """World transform of every joint frame (index 0: the universe) for one lane; `placement_p` `[njoints][3]` replaces
    the translations of the joint placements."""
    oMi = [np.eye(4)]
    for j in range(1, model.njoints):
        p = model.placement_p[j] if placement_p is None else placement_p[j]
        oMi.append(oMi[int(model.parents[j])] @ _hom(model.placement_R[j], p) @ joint_motion(model, j, q))
    return oMi


def jacobian_columns(model: CompiledModel, j: int, oMj: np.ndarray, p: np.ndarray) -> np.ndarray:
    """Columns `[6][nv_j]` (linear; angular, world frame) of joint j for a point p of the world."""
    t = int(model.jtypes[j])
    R, pj = oMj[:3, :3], oMj[:3, 3]
    revolute = lambda z: np.concatenate([np.cross(z, p - pj), z])      # noqa: E731
    prismatic = lambda z: np.concatenate([z, np.zeros(3)])              # noqa: E731
    if t == JT_FREEFLYER:
        return np.stack([prismatic(R[:, k]) for k in range(3)] + [revolute(R[:, k]) for k in range(3)], 1)
    if t == JT_SPHERICAL:
        return np.stack([revolute(R[:, k]) for k in range(3)], 1)
    z = R @ _axis(model, j)
    return (prismatic(z) if JT_PX <= t <= JT_PU else revolute(z))[:, None]


def frames(model: CompiledModel, frame_names: Sequence[str], q: np.ndarray, v: Optional[np.ndarray] = None,
           modes: Optional[Sequence[int]] = None, model_lane: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """`pose` `[7][K][B]`, `rot` `[K][B][3][3]`, `rpy` `[3][K][B]` (from the rotation matrix) and, with `v`, `vel` `[6][K][B]`
    of the named frames at `q` `[nq][B]`.  `model_lane` `[13 * njoints][B]`: per-lane joint placement translations."""
    K, B = len(frame_names), q.shape[1]
    modes = [LOCAL] * K if modes is None else list(modes)
    out = dict(pose=np.zeros((7, K, B)), rot=np.zeros((K, B, 3, 3)), rpy=np.zeros((3, K, B)))
    if v is not None:
        out["vel"] = np.zeros((6, K, B))
    for b in range(B):
        pp = None
        if model_lane is not None:
            pp = np.stack([model_lane[13 * j + 10:13 * j + 13, b] for j in range(model.njoints)])
        oMi = joint_transforms(model, q[:, b], pp)
        for k, name in enumerate(frame_names):
            fr = model.frame(name)
            M = oMi[int(fr.parent_joint)] @ _hom(fr.R, fr.p)
            R, p = M[:3, :3], M[:3, 3]
            out["pose"][:3, k, b], out["pose"][3:, k, b], out["rot"][k, b] = p, matrix_to_quat(R), R
            out["rpy"][:, k, b] = (np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], np.hypot(R[2, 1], R[2, 2])),
                                   np.arctan2(R[1, 0], R[0, 0]))
            if v is None:
                continue
            tw, j = np.zeros(6), int(fr.parent_joint)
            while j != 0:
                iv = int(model.idx_v[j])
                cols = jacobian_columns(model, j, oMi[j], p)
                tw += cols @ v[iv:iv + cols.shape[1], b]
                j = int(model.parents[j])
            if modes[k] != LOCAL_WORLD_ALIGNED:
                tw = np.concatenate([R.T @ tw[:3], R.T @ tw[3:]])
            out["vel"][:, k, b] = tw
    return out


def integrate_configuration(model: CompiledModel, q: np.ndarray, v: np.ndarray, eps: float) -> np.ndarray:
    """A configuration `[nq][B]` at distance `eps` along the velocity `v` (for finite differences of the pose)."""
    out = q.copy()

    def quat_step(quat: np.ndarray, w: np.ndarray) -> np.ndarray:
        th = np.linalg.norm(w)
        e = np.concatenate([np.sin(th / 2) * w / th, [np.cos(th / 2)]]) if th > 0 else np.array([0.0, 0.0, 0.0, 1.0])
        x, y, z, w_ = quat
        ex, ey, ez, ew = e
        return np.array([w_ * ex + x * ew + y * ez - z * ey, w_ * ey - x * ez + y * ew + z * ex,
                         w_ * ez + x * ey - y * ex + z * ew, w_ * ew - x * ex - y * ey - z * ez])

    for b in range(q.shape[1]):
        for j in range(1, model.njoints):
            t, iq, iv = int(model.jtypes[j]), int(model.idx_q[j]), int(model.idx_v[j])
            if t == JT_FREEFLYER:
                out[iq:iq + 3, b] += eps * _quat_matrix(q[iq + 3:iq + 7, b]) @ v[iv:iv + 3, b]
                out[iq + 3:iq + 7, b] = quat_step(q[iq + 3:iq + 7, b], eps * v[iv + 3:iv + 6, b])
            elif t == JT_SPHERICAL:
                out[iq:iq + 4, b] = quat_step(q[iq:iq + 4, b], eps * v[iv:iv + 3, b])
            elif JT_RUBX <= t <= JT_RUBU:
                a = np.arctan2(q[iq + 1, b], q[iq, b]) + eps * v[iv, b]
                out[iq, b], out[iq + 1, b] = np.cos(a), np.sin(a)
            else:
                out[iq, b] += eps * v[iv, b]
    return out


def finite_difference_velocity(model: CompiledModel, frame_names: Sequence[str], q: np.ndarray, v: np.ndarray, modes: Sequence[int],
                               eps: float, model_lane: Optional[np.ndarray] = None) -> np.ndarray:
    """Frame velocities `[6][K][B]` from a central difference of the numpy pose along `v`."""
    lo = frames(model, frame_names, integrate_configuration(model, q, v, -eps), model_lane=model_lane)
    hi = frames(model, frame_names, integrate_configuration(model, q, v, eps), model_lane=model_lane)
    mid = frames(model, frame_names, q, model_lane=model_lane)
    K, B = len(frame_names), q.shape[1]
    out = np.zeros((6, K, B))
    for k in range(K):
        for b in range(B):
            R = mid["rot"][k, b]
            pd = (hi["pose"][:3, k, b] - lo["pose"][:3, k, b]) / (2 * eps)
            S = (hi["rot"][k, b] - lo["rot"][k, b]) / (2 * eps) @ R.T
            w = 0.5 * np.array([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]])
            if modes[k] != LOCAL_WORLD_ALIGNED:
                pd, w = R.T @ pd, R.T @ w
            out[:3, k, b], out[3:, k, b] = pd, w
    return out


# --------------------------------------------------------------------------------------------------- the step average
def clamps(dtype) -> Tuple[np.floating, np.floating, np.floating]:
    """`tiny`, its square root and its power 2/3 in `dtype`: the clamps of log3 / exp3, log6 and exp6.  (The float32 root is
    rounded up so that its square is a normal number, as in the kernel.)"""
    dtype = np.dtype(dtype).type
    tiny = np.finfo(dtype).tiny
    if dtype is np.float64:
        return tiny, tiny ** (1 / 2), tiny ** (2 / 3)
    return dtype(tiny), np.nextafter(np.sqrt(dtype(tiny)), dtype(1)), dtype(float(tiny) ** (2 / 3))


def quat_multiply(l: np.ndarray, r: np.ndarray, sl: int = 1, sr: int = 1) -> np.ndarray:
    """`quat_multiply` with the four products of a component summed in pairs that cancel, as the kernel does: the conjugate of
    a quaternion times itself has an exactly zero vector part (the reference's left-to-right sum leaves a few 1e-18)."""
    (lx, ly, lz, lw), (rx, ry, rz, rw) = l, r
    lw, rw = l.dtype.type(sl) * lw, l.dtype.type(sr) * rw
    return np.stack([(lw * rx + lx * rw) + (ly * rz - lz * ry),
                     (lw * ry + ly * rw) + (lz * rx - lx * rz),
                     (lw * rz + lz * rw) + (lx * ry - ly * rx),
                     lw * rw - lx * rx - ly * ry - lz * rz])


def quat_apply(q: np.ndarray, u: np.ndarray, s: int = 1) -> np.ndarray:
    qx, qy, qz, qw = q
    s = q.dtype.type(s)
    xx, xy, xz, xw = qx * qx, qx * qy, qx * qz, qx * qw
    yy, yz, yw, zz, zw, ww = qy * qy, qy * qz, qy * qw, qz * qz, qz * qw, qw * qw
    x, y, z = u
    return np.stack([x * (xx + ww - yy - zz) + y * (2 * xy - 2 * s * zw) + z * (2 * xz + 2 * s * yw),
                     x * (2 * s * zw + 2 * xy) + y * (ww - xx + yy - zz) + z * (-2 * s * xw + 2 * yz),
                     x * (-2 * s * yw + 2 * xz) + y * (2 * s * xw + 2 * yz) + z * (ww - xx - yy + zz)])


def cross(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def remove_yaw(q: np.ndarray) -> np.ndarray:
    qx, qy, qz, qw = q
    one, half = q.dtype.type(1), q.dtype.type(0.5)
    cos_roll = one - 2 * (qx * qx + qy * qy)
    sin_roll = 2 * (qx * qw + qy * qz)
    cos_roll = cos_roll / np.sqrt(cos_roll * cos_roll + sin_roll * sin_roll)
    cos_roll_2 = np.sqrt(half * (one + cos_roll))
    sin_roll_2 = np.sign(sin_roll) * np.sqrt(half * (one - cos_roll))
    sin_pitch = 2 * (qy * qw - qx * qz)
    cos_pitch = np.sqrt(one - sin_pitch * sin_pitch)
    cos_pitch_2 = np.sqrt(half * (one + cos_pitch))
    sin_pitch_2 = np.sign(sin_pitch) * np.sqrt(half * (one - cos_pitch))
    return np.stack([sin_roll_2 * cos_pitch_2, cos_roll_2 * sin_pitch_2, -sin_roll_2 * sin_pitch_2, cos_roll_2 * cos_pitch_2])


def average_step(pose_prev: np.ndarray, pose: np.ndarray, inv_step_dt: float, modes: Sequence[int]) -> Dict[str, np.ndarray]:
    """One step average of poses `[7][K][B]` in their own dtype: `diff` `[6][K][B]`, `v_avg` `[6][K][B]`, `pose_mean` `[7][K][B]`,
    `quat_no_yaw` `[4][K][B]`; the order of operations of utils/math.py (`xyzquat_difference`, `log6`, `log3`, `exp6`, `exp3`,
    `remove_yaw_from_quat`) and of the `refresh` bodies of the quantity classes."""
    T = pose.dtype.type
    assert pose_prev.dtype == pose.dtype
    tiny, root, pow23 = clamps(pose.dtype)
    half, one = T(0.5), T(1)
    x0, q0, x1, q1 = pose_prev[:3], pose_prev[3:], pose[:3], pose[3:]
    with np.errstate(over="ignore"):
        pos = quat_apply(q0, x1 - x0, -1)
        qd = quat_multiply(q0, q1, -1, 1)
        sin_2 = np.sqrt(qd[0] * qd[0] + qd[1] * qd[1] + qd[2] * qd[2])
        theta = 2 * np.arctan2(sin_2, np.abs(qd[3]))
        ang = (theta / np.maximum(sin_2, tiny)) * qd[:3] * np.sign(qd[3])
        cot_2 = np.abs(qd[3]) / np.maximum(sin_2, root)
        theta = np.maximum(theta, root)
        beta = one / (theta * theta) - half * cot_2 / theta
        wxv = cross(ang, pos)
        w2xv = cross(ang, wxv)
        lin = pos - half * wxv + beta * w2xv
        vl, va = -half * lin, -half * ang
        sum_sq = va[0] * va[0] + va[1] * va[1] + va[2] * va[2]
        theta_sq = np.maximum(sum_sq, pow23)
        th = np.sqrt(theta_sq)
        alpha_wxv = (one - np.cos(th)) / theta_sq
        alpha_w2 = (th - np.sin(th)) / theta_sq / th
        wxv = cross(va, vl)
        w2xv = cross(va, wxv)
        te = vl + alpha_wxv * wxv + alpha_w2 * w2xv
        th3 = np.sqrt(sum_sq)
        axis = va / np.maximum(th3, tiny)
        qe = np.concatenate([np.sin(half * th3) * axis, np.cos(half * th3)[None]])
        xm = x1 + quat_apply(q1, te)
        qm = quat_multiply(q1, qe)
        qny = remove_yaw(qm)
        diff = np.concatenate([lin, ang])
        inv = T(inv_step_dt)
        l, g = inv * lin, inv * ang
        for k, mode in enumerate(modes):
            if mode != LOCAL:
                r = qny[:, k] if mode == ODOMETRY else qm[:, k]
                l[:, k], g[:, k] = quat_apply(r, l[:, k]), quat_apply(r, g[:, k])
    out = dict(diff=diff, v_avg=np.concatenate([l, g]), pose_mean=np.concatenate([xm, qm]), quat_no_yaw=qny)
    assert all(a.dtype == pose.dtype for a in out.values())
    return out
