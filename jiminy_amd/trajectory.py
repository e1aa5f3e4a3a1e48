"""Host side of the reference trajectories block: recorded trajectories as plain arrays, and from a model and a dataset of
them to the plan `jm_block_trajectory_state` interprets on the device.

Reference: `Trajectory` of python/jiminy_py/src/jiminy_py/dynamics.py (:150-388: the constructor's checks, `time_interval`,
the stride `log6(M_end * M_start^-1)` of the free-flyer, :207-213) and `DatasetTrajectoryQuantity` of
python/gym_jiminy/common/gym_jiminy/common/bases/quantities.py (:870-1210: the ordered registry of named trajectories with a
time mode each, the selection and `time_offset = t_start + ratio * (t_end - t_start)`, :1171-1174).  The stride is computed here
once, in float64, with `log6` of gym_jiminy/common/utils/math.py (:842-894) restated in numpy.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from . import _abi
from ._plan import AXIS_KIND, SEG_FREEFLYER, SEG_PAXIS, SEG_PX, SEG_QUAT, SEG_UNBOUNDED, fill_desc
from .model import (JT_FREEFLYER, JT_PU, JT_PX, JT_PY, JT_PZ, JT_RUBU, JT_RUBX, JT_RUBY, JT_RUBZ, JT_SPHERICAL,
                    CompiledModel)

# time modes (`TrajectoryTimeMode`, dynamics.py:147)
RAISE, WRAP, CLIP = 0, 1, 2
MODES = {"raise": RAISE, "wrap": WRAP, "clip": CLIP}
# bits of `fields`, of the flags of `status`; rows of `status`
HAS_V, HAS_A, HAS_COMMAND = 1, 2, 4
FLAG_OUT_OF_RANGE, FLAG_BAD_TRAJECTORY = 1, 2
STATUS = ("flags", "n_steps", "index")
# state fields of the reference's `State` that a trajectory here cannot carry
UNSUPPORTED_FIELDS = ("u", "f_external", "lambda_c")


def time_mode(mode: Union[int, str]) -> int:
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"unknown time mode '{mode}' (one of {', '.join(MODES)})")
        return MODES[mode]
    if int(mode) not in MODES.values():
        raise ValueError(f"unknown time mode {mode} (0 raise, 1 wrap, 2 clip)")
    return int(mode)


class Trajectory:
    """A recorded trajectory of the engine's model as plain arrays: `t [S]` (float64, not decreasing: two equal consecutive
    times are t-, t+), `q [S][nq]` and optionally `v`, `a` `[S][nv]`, `command [S][n_motors]`.  ≙ `Trajectory(states, robot,
    use_theoretical_model)`; a field is given for every sample or not at all."""

    def __init__(self, t, q, v=None, a=None, command=None, **unsupported) -> None:
        for name in unsupported:
            if name in UNSUPPORTED_FIELDS:
                raise NotImplementedError(f"the state field '{name}' is not part of a device-resident trajectory")
            raise TypeError(f"unexpected field '{name}'")
        self.t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        if self.t.size < 2:
            raise ValueError("a trajectory needs at least 2 samples")
        if not np.all(np.isfinite(self.t)):
            raise ValueError("the times of a trajectory must be finite")
        if np.any(np.diff(self.t) < 0.0):
            raise ValueError("Time must not be decreasing between consecutive timesteps.")     # (dynamics.py:196-199)
        self.q = self._field("q", q)
        self.v = None if v is None else self._field("v", v)
        self.a = None if a is None else self._field("a", a)
        self.command = None if command is None else self._field("command", command)
        if self.v is not None and self.a is not None and self.a.shape != self.v.shape:
            raise ValueError("v and a must have the same shape")

    def _field(self, name: str, value) -> np.ndarray:
        value = np.ascontiguousarray(value, dtype=np.float64)
        if value.ndim != 2 or value.shape[0] != self.t.size or value.shape[1] < 1:
            raise ValueError(f"{name} must have shape [{self.t.size}][rows]")
        if not np.all(np.isfinite(value)):
            raise ValueError(f"{name} must be finite")
        return value

    @property
    def num_samples(self) -> int:
        return int(self.t.size)

    @property
    def fields(self) -> int:
        return (HAS_V if self.v is not None else 0) | (HAS_A if self.a is not None else 0) | \
               (HAS_COMMAND if self.command is not None else 0)

    @property
    def time_interval(self) -> Tuple[float, float]:
        return float(self.t[0]), float(self.t[-1])


def _quat_mul(l: np.ndarray, r: np.ndarray) -> np.ndarray:
    return np.array([l[3] * r[0] + l[0] * r[3] + l[1] * r[2] - l[2] * r[1],
                     l[3] * r[1] - l[0] * r[2] + l[1] * r[3] + l[2] * r[0],
                     l[3] * r[2] + l[0] * r[1] - l[1] * r[0] + l[2] * r[3],
                     l[3] * r[3] - l[0] * r[0] - l[1] * r[1] - l[2] * r[2]])


def _quat_apply(q: np.ndarray, u: np.ndarray) -> np.ndarray:
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R @ u


def log6(xyzquat: np.ndarray) -> np.ndarray:
    """`log6` of utils/math.py (:866-890, with `log3`, :757-770) for one pose, float64: (linear, angular)."""
    pos, quat = np.asarray(xyzquat[:3], dtype=np.float64), np.asarray(xyzquat[3:], dtype=np.float64)
    tiny = np.finfo(np.float64).tiny
    sin_2 = np.sqrt(np.sum(np.square(quat[:3])))
    theta = 2 * np.arctan2(sin_2, np.abs(quat[3]))
    ang = theta / np.maximum(sin_2, tiny) * quat[:3] * np.sign(quat[3])
    eps = tiny ** (1 / 2)
    cot_2 = np.abs(quat[3]) / np.maximum(sin_2, eps)
    theta = np.maximum(theta, eps)
    beta = 1.0 / np.square(theta) - 0.5 * cot_2 / theta
    wxv = np.cross(ang, pos)
    return np.concatenate((pos - 0.5 * wxv + beta * np.cross(ang, wxv), ang))


def stride_of(q_start: np.ndarray, q_end: np.ndarray) -> np.ndarray:
    """`log6(M_end * M_start.inverse())` of the free-flyer rows (dynamics.py:211-213)."""
    inv = np.array([-q_start[3], -q_start[4], -q_start[5], q_start[6]]) / np.sum(np.square(q_start[3:7]))
    quat = _quat_mul(np.asarray(q_end[3:7]), inv)
    pos = np.asarray(q_end[:3]) - _quat_apply(quat, np.asarray(q_start[:3]))
    return log6(np.concatenate((pos, quat)))


def joint_table(model: CompiledModel) -> Tuple[List[int], List[int]]:
    """Kind and first `q` row of every joint of the model, the kinds of the frame kinematics plan."""
    kinds, rows = [], []
    for j in range(1, int(model.njoints)):
        t = int(model.jtypes[j])
        if t in AXIS_KIND:
            kind = AXIS_KIND[t]
        elif t in (JT_RUBX, JT_RUBY, JT_RUBZ, JT_RUBU):
            kind = SEG_UNBOUNDED
        elif t in (JT_PX, JT_PY, JT_PZ):
            kind = SEG_PX + (t - JT_PX)
        elif t == JT_PU:
            kind = SEG_PAXIS
        elif t == JT_SPHERICAL:
            kind = SEG_QUAT
        elif t == JT_FREEFLYER:
            kind = SEG_FREEFLYER
        else:
            raise NotImplementedError(f"joint type {t} of joint '{model.joint_names[j]}'")
        kinds.append(kind)
        rows.append(int(model.idx_q[j]))
    return kinds, rows


def make_desc(*, dtype, sample_start, times, mode, stride, data, nq: int, nv: int, n_command: int, fields: int, joint_kind,
              joint_q_index, motor_q_index) -> Tuple["_abi.TrajectoryDesc", List[np.ndarray]]:
    """`jm_trajectory_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive.  `data` is
    `[S][R]`, converted to `dtype`; `stride` may be None (no free-flyer), so may `motor_q_index`."""
    d = _abi.TrajectoryDesc()
    ints = dict(sample_start=sample_start, mode=mode, joint_kind=joint_kind, joint_q_index=joint_q_index)
    if motor_q_index is not None and len(motor_q_index):
        ints["motor_q_index"] = motor_q_index
    dbls = dict(times=times)
    if stride is not None:
        dbls["stride"] = stride
    a, keep = fill_desc(d, ints, dbls)
    np_dtype = np.dtype(dtype)
    samples = np.ascontiguousarray(data, dtype=np_dtype)
    keep.append(samples)
    d.data = samples.ctypes.data
    d.dtype = _abi.JM_F64 if np_dtype == np.float64 else _abi.JM_F32
    d.n_trajectories, d.n_samples = len(a["mode"]), len(a["times"])
    d.nq, d.nv, d.n_command, d.fields = int(nq), int(nv), int(n_command), int(fields)
    d.n_joints, d.n_motors = len(a["joint_kind"]), len(a.get("motor_q_index", ()))
    return d, keep


@dataclass
class TrajectoryPlan:
    names: List[str]
    modes: List[int]
    time_interval: np.ndarray                    # [N][2] float64
    fields: int
    has_freeflyer: bool
    nq: int
    nv: int
    n_command: int
    n_motors: int
    arrays: Dict[str, Any] = field(default_factory=dict)
    dtype: Any = np.float64                      # of the samples on the device: the block sets its engine's

    @property
    def n_trajectories(self) -> int:
        return len(self.names)

    def desc(self, dtype=None) -> Tuple["_abi.TrajectoryDesc", List[np.ndarray]]:
        return make_desc(dtype=dtype or self.dtype, **self.arrays)


def _check_quaternions(name: str, q: np.ndarray, kinds: Sequence[int], rows: Sequence[int]) -> None:
    for kind, row in zip(kinds, rows):
        if kind not in (SEG_QUAT, SEG_FREEFLYER):
            continue
        quat = q[:, row + 3:row + 7] if kind == SEG_FREEFLYER else q[:, row:row + 4]
        dots = np.sum(quat[1:] * quat[:-1], axis=1)
        if np.any(dots < 0.0):
            raise ValueError(f"trajectory '{name}': consecutive quaternions at q row {row} have a negative dot product (sample "
                             f"{int(np.argmax(dots < 0.0)) + 1}); flip the sign of one of them, both stand for the same rotation")


def build_plan(model: CompiledModel, dataset: Mapping[str, Tuple[Trajectory, Union[int, str]]],
               motor_q_index: Optional[Sequence[int]] = None) -> TrajectoryPlan:
    """The plan of a dataset `{name: (Trajectory, mode)}`, in its order, for `model`.  Every trajectory carries the same
    optional fields.  `motor_q_index`: the `q` rows of the motors (default: those of `model.motors`)."""
    if not dataset:
        raise ValueError("the dataset needs at least one trajectory")
    kinds, rows = joint_table(model)
    nq, nv, n_command = int(model.nq), int(model.nv), len(model.motors)
    if motor_q_index is None:
        one_row = {r for k, r in zip(kinds, rows) if k not in (SEG_UNBOUNDED, SEG_QUAT, SEG_FREEFLYER)}
        motor_q_index = [int(m.idx_q) for m in model.motors if int(m.idx_q) in one_row]
    has_freeflyer = bool(kinds) and kinds[0] == SEG_FREEFLYER
    names, modes, fields_, blocks, times, strides, start = [], [], None, [], [], [], [0]
    for name, entry in dataset.items():
        try:
            traj, mode = entry
        except (TypeError, ValueError):
            raise ValueError(f"trajectory '{name}': expected a pair (Trajectory, mode)") from None
        if not isinstance(traj, Trajectory):
            raise ValueError(f"trajectory '{name}': expected a jiminy_amd.trajectory.Trajectory")
        if traj.q.shape[1] != nq:
            raise ValueError(f"trajectory '{name}': q has {traj.q.shape[1]} rows, the model {nq}")
        for what, value, n in (("v", traj.v, nv), ("a", traj.a, nv), ("command", traj.command, n_command)):
            if value is not None and value.shape[1] != n:
                raise ValueError(f"trajectory '{name}': {what} has {value.shape[1]} rows, the model {n}")
        if fields_ is None:
            fields_ = traj.fields
        elif traj.fields != fields_:
            raise ValueError(f"trajectory '{name}' carries other optional fields than the first one of the dataset")
        _check_quaternions(name, traj.q, kinds, rows)
        names.append(str(name))
        modes.append(time_mode(mode))
        blocks.append(np.concatenate([x for x in (traj.q, traj.v, traj.a, traj.command) if x is not None], axis=1))
        times.append(traj.t)
        strides.append(stride_of(traj.q[0], traj.q[-1]) if has_freeflyer else np.zeros(6))
        start.append(start[-1] + traj.num_samples)
    arrays = dict(sample_start=start, times=np.concatenate(times), mode=modes, stride=np.array(strides) if has_freeflyer else None,
                  data=np.concatenate(blocks, axis=0), nq=nq, nv=nv, n_command=n_command, fields=fields_, joint_kind=kinds,
                  joint_q_index=rows, motor_q_index=list(motor_q_index))
    return TrajectoryPlan(names=names, modes=modes, time_interval=np.array([[t[0], t[-1]] for t in times], dtype=np.float64),
                          fields=int(fields_), has_freeflyer=has_freeflyer, nq=nq, nv=nv, n_command=n_command,
                          n_motors=len(motor_q_index), arrays=arrays)
