"""Test-side numpy of the attitude observers (tests only): a straight restatement of the three kernels of
jiminy_amd/csrc/jm_attitude.h, vectorised over the lanes, in float64 or float32 -- what rounding alone does to the
reference's formulas.  The tests take the float32 bounds from it and drive the environment test with it.

Arrays as the kernels see them: imu `[n_imu][6][B]` (gyro 0-2, accel 3-5), quat `[4][n_imu][B]` (xyzw), omega / bias / cf / rpy
`[3][n_imu][B]`, twist `[n_imu][B]`, q `[nq][B]`.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from tests.deformation_numpy import _mat_to_quat, _mm, _qmul, _renorm, _swing, _joint_rotation, quat_to_rot

SEG_NONE, SEG_X, SEG_Y, SEG_Z, SEG_AXIS, SEG_UNBOUNDED, SEG_QUAT = range(7)


def tilt(q: np.ndarray) -> np.ndarray:
    f = q.dtype.type
    return np.array([f(2) * (q[0] * q[2] - q[1] * q[3]), f(2) * (q[1] * q[2] + q[3] * q[0]), f(1) - f(2) * (q[0] * q[0] + q[1] * q[1])])


def rpy_of(quat: np.ndarray) -> np.ndarray:
    f = quat.dtype.type
    x, y, z, w = quat
    n2 = (f(3) - (x * x + y * y + z * z + w * w)) / f(2)
    yw, xz = y * w * n2, x * z * n2
    with np.errstate(invalid="ignore"):
        return np.array([np.arctan2(f(2) * (x * w + y * z), f(1) - f(2) * (x * x + y * y)),
                         -f(np.pi) / f(2) + f(2) * np.arctan2(np.sqrt(f(1) + f(2) * (yw - xz)), np.sqrt(f(1) - f(2) * (yw - xz))),
                         np.arctan2(f(2) * (z * w + x * y), f(1) - f(2) * (y * y + z * z))]).astype(quat.dtype)


def remove_twist(quat: np.ndarray) -> np.ndarray:
    """`remove_twist_from_quat` on `[4][n_imu][B]`: the singular flag is taken over the IMUs of a lane."""
    f = quat.dtype.type
    v = tilt(quat)                                                  # [3][n_imu][B]
    singular = np.any(v[2] < f(-1) + f(1e-5), axis=0)
    return np.stack([_swing(v[:, s], singular) for s in range(quat.shape[1])], 1).astype(quat.dtype)


def mahony_tick(quat, bias, imu, kp, ki, dt: float, ignore_twist: bool, dtype=np.float64):
    """One refresh of an initialised filter.  Returns quat, bias, omega, cf (new arrays)."""
    f = np.dtype(dtype).type
    quat, bias, imu = np.asarray(quat, dtype), np.asarray(bias, dtype), np.asarray(imu, dtype)
    kp, ki, step = np.asarray(kp, dtype)[None, :, None], np.asarray(ki, dtype)[None, :, None], f(dt)
    gyro, acc = imu[:, :3].transpose(1, 0, 2), imu[:, 3:].transpose(1, 0, 2)
    v = tilt(quat)
    omega = gyro - bias
    a = acc / f(9.81)
    mes = np.array([a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0]])
    cf = omega + kp * mes
    moving = ~(np.abs(cf) < f(1e-6)).all(axis=(0, 1))               # [B]
    with np.errstate(all="ignore"):
        theta = np.sqrt(cf[0] * cf[0] + cf[1] * cf[1] + cf[2] * cf[2])
        axis = cf / theta
        half = theta * (step / f(2))
        p, pw = axis * np.sin(half), np.cos(half)
        x, y, z, w = quat
        new = _renorm(np.array([x * pw + w * p[0] - z * p[1] + y * p[2], y * pw + z * p[0] + w * p[1] - x * p[2],
                                z * pw - y * p[0] + x * p[1] + w * p[2], w * pw - x * p[0] - y * p[1] - z * p[2]]))
        quat = np.where(moving, new, quat).astype(dtype)
        bias = np.where(moving, bias - ki * step * mes, bias).astype(dtype)
    if ignore_twist:
        quat = remove_twist(quat)
    return quat, bias, omega.astype(dtype), cf.astype(dtype)


def body_tick(imu_quat, imu_omega, rel_quat, twist, twist_mode: int, time_constant_inv: float, dt: float, dtype=np.float64):
    """`BodyObserver.refresh_observation`.  rel_quat `[n_imu][4]`.  Returns quat, omega, twist."""
    f = np.dtype(dtype).type
    iq, io = np.asarray(imu_quat, dtype), np.asarray(imu_omega, dtype)
    rel = np.asarray(rel_quat, dtype).T[:, :, None]                 # [4][n_imu][1]
    quat = _qmul(iq, np.broadcast_to(rel, iq.shape), 1, -1).astype(dtype)
    xx, xy, xz, xw = rel[0] * rel[0], rel[0] * rel[1], rel[0] * rel[2], rel[0] * rel[3]
    yy, yz, yw = rel[1] * rel[1], rel[1] * rel[2], rel[1] * rel[3]
    zz, zw, ww = rel[2] * rel[2], rel[2] * rel[3], rel[3] * rel[3]
    x, y, z = io
    two = f(2)
    omega = np.array([x * (xx + ww - yy - zz) + y * (two * xy - two * zw) + z * (two * xz + two * yw),
                      x * (two * zw + two * xy) + y * (ww - xx + yy - zz) + z * (-two * xw + two * yz),
                      x * (-two * yw + two * xz) + y * (two * xw + two * yz) + z * (ww - xx - yy + zz)]).astype(dtype)
    twist = np.asarray(twist, dtype)
    if twist_mode:
        quat = remove_twist(quat)
    if twist_mode == 2:
        qx, qy, _, qw = quat
        dtwist = (-qy * omega[0] + qx * omega[1]) / qw + omega[2]
        twist = twist * f(max(0.0, 1.0 - time_constant_inv * dt)) + dtwist * f(dt)
        pz, pw = np.sin(f(0.5) * twist), np.cos(f(0.5) * twist)
        quat = np.array([pw * qx - pz * qy, pz * qx + pw * qy, pz * qw, pw * qw]).astype(dtype)
    return quat, omega, twist.astype(dtype)


def frame_rotations(arrays: Dict[str, np.ndarray], q: np.ndarray, dtype=np.float64) -> np.ndarray:
    """World rotation of every IMU frame of a plan, `[n_imu][3][3][B]`."""
    q = np.asarray(q, dtype)
    Bn = q.shape[-1]
    start = np.asarray(arrays["frame_seg_start"]).reshape(-1)
    kind, qi = np.asarray(arrays["seg_kind"]).reshape(-1), np.asarray(arrays["seg_q_index"]).reshape(-1)
    rot = np.asarray(arrays["seg_rot"], dtype).reshape(-1, 3, 3)
    axis = np.asarray(arrays["seg_axis"], dtype).reshape(-1, 3)
    out = []
    for s in range(len(start) - 1):
        R = np.broadcast_to(np.eye(3, dtype=dtype)[:, :, None], (3, 3, Bn))
        for g in range(start[s], start[s + 1]):
            R = _mm(R, np.broadcast_to(rot[g][:, :, None], (3, 3, Bn)))
            k, i = int(kind[g]), int(qi[g])
            if k in (SEG_X, SEG_Y, SEG_Z, SEG_AXIS):
                R = _mm(R, _joint_rotation(k, axis[g], q[i]))
            elif k == SEG_UNBOUNDED:
                a, c, sn = axis[g], q[i], q[i + 1]
                K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=dtype)
                J = np.eye(3, dtype=dtype)[:, :, None] * c + K[:, :, None] * sn + np.outer(a, a).astype(dtype)[:, :, None] * (1 - c)
                R = _mm(R, J.astype(dtype))
            elif k == SEG_QUAT:
                R = _mm(R, quat_to_rot(q[i:i + 4]).astype(dtype))
        out.append(R)
    return np.array(out)


def init(arrays: Dict[str, np.ndarray], q, imu, exact_init: bool, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """The first refresh of an episode.  Returns quat `[4][n_imu][B]` and the mask of the lanes that took the exact path."""
    f = np.dtype(dtype).type
    imu = np.asarray(imu, dtype)
    R = frame_rotations(arrays, q, dtype)
    exact_q = np.stack([_mat_to_quat(R[s]) for s in range(R.shape[0])], 1).astype(dtype)
    Bn = imu.shape[-1]
    if exact_init:
        return exact_q, np.ones(Bn, dtype=bool)
    acc = imu[:, 3:].transpose(1, 0, 2)                             # [3][n_imu][B]
    falling = (np.abs(acc) < f(0.1 * 9.81)).all(axis=(0, 1))
    with np.errstate(all="ignore"):
        v = acc / np.sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2])
        singular = np.any(v[2] < f(-1) + f(1e-5), axis=0)
        swing = np.stack([_swing(v[:, s], singular) for s in range(acc.shape[1])], 1)
    return np.where(falling, exact_q, swing).astype(dtype), falling
