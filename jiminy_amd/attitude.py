"""Host side of the attitude observers (`MahonyFilter` with its options, `BodyObserver`): from a `CompiledModel` to the plan
`jm_block_attitude_init` / `jm_block_mahony_observer` / `jm_block_body_observer` interpret on the device.

Reference: python/gym_jiminy/common/gym_jiminy/common/blocks/mahony_filter.py -- `MahonyFilter.__init__` (:138-226:
per-IMU gains, a float is repeated for every IMU) and the exact initialisation of `refresh_observation` (:356-368: the
world rotation `oMf` of every IMU frame); blocks/body_orientation_observer.py -- `BodyObserver.__init__` (:168-173: the
rotation of every IMU frame relative to its parent body, as a quaternion by `matrices_to_quat`).

The world rotation of a sensor frame is a walk from the root to the frame over the configuration: per IMU a list of
segments, each a constant rotation (joint placements, the frame's own rotation) followed by the rotation of one joint
read from `q` -- by its angle, by (cos, sin) for an unbounded revolute joint, or as a unit quaternion for a spherical joint
and the orientation of a free-flyer.  Prismatic joints contribute nothing.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Sequence, Tuple, Union

import numpy as np

from . import _abi
from ._plan import (AXIS_KIND, SEG_AXIS, SEG_NONE, SEG_QUAT, SEG_UNBOUNDED, SEG_X, SEG_Y, SEG_Z, SegmentTable,  # noqa: F401
                    fill_desc)
from .model import JT_FREEFLYER, JT_PU, JT_PX, JT_RUBU, JT_RUBX, JT_RUBY, JT_RUBZ, JT_SPHERICAL, CompiledModel

TWIST_KEEP, TWIST_REMOVE, TWIST_INTEGRATE = 0, 1, 2


def matrix_to_quat(m: np.ndarray) -> np.ndarray:
    """One rotation matrix to a quaternion xyzw by the branch rule of `matrices_to_quat` (utils/math.py:327-356)."""
    if m[2, 2] < 0:
        if m[0, 0] > m[1, 1]:
            t = 1 + m[0, 0] - m[1, 1] - m[2, 2]
            q = [t, m[1, 0] + m[0, 1], m[0, 2] + m[2, 0], m[2, 1] - m[1, 2]]
        else:
            t = 1 - m[0, 0] + m[1, 1] - m[2, 2]
            q = [m[1, 0] + m[0, 1], t, m[2, 1] + m[1, 2], m[0, 2] - m[2, 0]]
    else:
        if m[0, 0] < -m[1, 1]:
            t = 1 - m[0, 0] - m[1, 1] + m[2, 2]
            q = [m[0, 2] + m[2, 0], m[2, 1] + m[1, 2], t, m[1, 0] - m[0, 1]]
        else:
            t = 1 + m[0, 0] + m[1, 1] + m[2, 2]
            q = [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], t]
    return np.asarray(q, dtype=np.float64) / (2 * np.sqrt(t))


def broadcast_gain(gain: Union[np.ndarray, Sequence[float], float], n_imu: int) -> np.ndarray:
    """≙ mahony_filter.py:176-186: a float is repeated for every IMU, anything else is taken as an array over them."""
    if isinstance(gain, (float, int)):
        gain = (float(gain),) * n_imu
    out = np.asarray(gain, dtype=np.float64)
    if out.shape != (n_imu,):
        raise ValueError(f"expected one gain or one gain per IMU ({n_imu}), got an array of shape {out.shape}")
    return out


@dataclass
class AttitudePlan:
    imu_names: List[str]
    kp: np.ndarray
    ki: np.ndarray
    rel_quat: np.ndarray                         # [n_imu][4] ≙ `BodyObserver._imu_rel_quats` (transposed)
    arrays: Dict[str, Any] = field(default_factory=dict)

    @property
    def n_imu(self) -> int:
        return len(self.imu_names)

    def desc(self) -> Tuple["_abi.AttitudeDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(*, nq: int, kp, ki, rel_quat, frame_seg_start, seg_kind, seg_q_index, seg_rot, seg_axis
              ) -> Tuple["_abi.AttitudeDesc", List[np.ndarray]]:
    """`jm_attitude_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.AttitudeDesc()
    a, keep = fill_desc(d, dict(frame_seg_start=frame_seg_start, seg_kind=seg_kind, seg_q_index=seg_q_index),
                        dict(kp=kp, ki=ki, rel_quat=rel_quat, seg_rot=seg_rot, seg_axis=seg_axis))
    d.n_imu, d.nq, d.n_seg = len(a["kp"]), int(nq), len(a["seg_kind"])
    return d, keep


def build_plan(model: CompiledModel, kp: Union[np.ndarray, Sequence[float], float] = 1.0,
               ki: Union[np.ndarray, Sequence[float], float] = 0.1) -> AttitudePlan:
    """The plan of the attitude observers for every `ImuSensor` of the compiled model, in sensor order."""
    sensors = model.sensors.get("ImuSensor", [])
    if not sensors:
        raise ValueError("the attitude observers need at least one ImuSensor")
    n_imu = len(sensors)
    kp, ki = broadcast_gain(kp, n_imu), broadcast_gain(ki, n_imu)
    segs = SegmentTable()

    def joint_segment(j: int):
        t, iq = int(model.jtypes[j]), int(model.idx_q[j])
        if t in AXIS_KIND:
            return AXIS_KIND[t], iq, model.axes[j], 0.0
        if t in (JT_RUBX, JT_RUBY, JT_RUBZ, JT_RUBU):
            return SEG_UNBOUNDED, iq, model.axes[j] if t == JT_RUBU else np.eye(3)[t - JT_RUBX], 0.0
        if t == JT_SPHERICAL:
            return SEG_QUAT, iq, np.zeros(3), 0.0
        if t == JT_FREEFLYER:
            return SEG_QUAT, iq + 3, np.zeros(3), 0.0
        if not JT_PX <= t <= JT_PU:
            raise NotImplementedError(f"joint type {t} of joint '{model.joint_names[j]}'")
        return None

    rel_quat = []
    for s in sensors:
        fr = model.frame(s["frame"])
        rel_quat.append(matrix_to_quat(np.asarray(fr.R, dtype=np.float64)))
        segs.add_frame(model, int(fr.parent_joint), fr.R, joint_segment)
    arrays = dict(nq=int(model.nq), kp=kp, ki=ki, rel_quat=np.array(rel_quat), frame_seg_start=segs.frame_seg_start,
                  seg_kind=segs.kind, seg_q_index=segs.index, seg_rot=np.array(segs.rot), seg_axis=np.array(segs.axis))
    return AttitudePlan(imu_names=[s["name"] for s in sensors], kp=kp, ki=ki, rel_quat=np.array(rel_quat), arrays=arrays)
