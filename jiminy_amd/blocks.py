"""Batched, device-resident versions of the gym_jiminy pipeline blocks used by the ANYmal/Atlas
environments: PD controller + ZOH command integrator, PD adapter and
Mahony attitude filter.

They restate the numba kernels of the reference
(python/gym_jiminy/common/gym_jiminy/common/blocks/proportional_derivative_controller.py:22-260,
mahony_filter.py:28-101) over `[rows][B]` arrays; every lane is one environment.

Two forms of the per-controller-tick blocks:
* `HipBlocks.pd_controller` / `HipBlocks.mahony_filter`: ONE hand-written HIP kernel launch each
  (csrc/jm_blocks.h behind `jm_block_*` of include/jiminy_hip.h) -- what the environments use;
* `pd_controller` / `mahony_filter` / `integrate_zoh`: the same arithmetic as elementwise tensor
  programs (scalar branches become `torch.where`), ~40 launches per block.  They run wherever their
  tensors live and serve as the readable specification the kernels are tested against.
`HipBlocks.pd_adapter` / `HipBlocks.motor_safety_limit` are the `PDAdapter` / `MotorSafetyLimit` blocks as single
launches; `pd_adapter` below is the tensor-program form.

`DeformationEstimator` is the observer block of that name (blocks/deformation_estimator.py): one HIP launch
(csrc/jm_deform.h behind `jm_block_deformation_estimator`) driven by a plan that jiminy_amd/deformation.py builds on the host.
It has no tensor-program form: its specification is the reference's own output (tests/golden/ref_deformation.npz).

`MahonyFilter` and `BodyObserver` are the observer blocks of those names with every option of the reference's classes
(blocks/mahony_filter.py:104-393, blocks/body_orientation_observer.py:74-266): per-IMU gains, twist removal, Euler angles, the
initialisation at the first refresh of an episode, the body frames and the leaky twist integrator.  One HIP launch per
refresh (csrc/jm_attitude.h) driven by a plan that jiminy_amd/attitude.py builds; specification: tests/golden/ref_attitude.npz.

`FrameKinematics` gives the pose and the velocity of named frames and their SE3 average over an environment step (what the
reference's quantity layer reads from `pinocchio_data.oMf` and `getFrameVelocity`): one HIP launch each (csrc/jm_frames.h) driven
by a plan that jiminy_amd/frames.py builds; specification of the average: tests/golden/ref_frames.npz.

`LocomotionQuantities` gives the balance quantities of a legged robot (centre of mass, odometry pose, ZMP, capture point, base
momentum, normalised contact and foot forces, the scalars of two rewards and two terminations) from what a step left on the
device and from the tensors of a `FrameKinematics`: one HIP launch per refresh (csrc/jm_locomotion.h) driven by a plan that
jiminy_amd/locomotion.py builds; specification: tests/golden/ref_locomotion.npz.

`ActuatedJointQuantities` gives the actuated-joint part of the quantity layer (joint kinematics in motor order, distances to
the mechanical stops, the mechanical-safety count, the mechanical power, its sliding average over environment steps and the
reward on it) from the engine's `q / v / a / command`: one HIP launch per refresh (csrc/jm_actuation.h) driven by a plan that
jiminy_amd/actuation.py builds; specification: tests/golden/ref_actuation.npz.

`FootPoseQuantities` gives the mean pose of the feet (position mean and quaternion average: a copy, a midpoint or the dominant
eigenvector of a 4 x 4 matrix per lane), its odometry pose, the poses of the feet relative to it and the tracking error and
rewards against a reference of those relative poses, from the `pose` of a `FrameKinematics`: one HIP launch per refresh
(csrc/jm_footposes.h) driven by a plan that jiminy_amd/footposes.py builds; specification: tests/golden/ref_footposes.npz.

`TrackingWindows` gives the drift of the odometry pose and the shift of the relative foot poses and of the motor positions
against a reference motion over sliding windows of environment steps, and the reward on the drift, from the tensors of the
three blocks above: one HIP launch per refresh (csrc/jm_tracking.h) driven by a plan that jiminy_amd/tracking.py builds;
specification: tests/golden/ref_tracking.npz.

`ReferenceTrajectory` gives the state of a recorded trajectory at every lane's own time (a device-resident dataset, a per-lane
selection and time offset; time modes, bisection, Lie-group interpolation, wrap odometry): the reference side of the four
blocks above.  One HIP launch per query (csrc/jm_trajectory.h) driven by a plan that jiminy_amd/trajectory.py builds;
specification: tests/golden/ref_trajectory.npz.

`CentroidalState` gives the centre of mass, the centroidal momentum and its time derivative of any state `(q, v, a)` -- the
state of a reference trajectory, for which the physics kernels leave no `centroidal` rows -- on the nominal model: one HIP
launch per refresh (csrc/jm_centroidal.h) driven by a plan that jiminy_amd/centroidal.py builds; specification: the oracle's
`centroidal` rows.  `LocomotionQuantities(state=(q, centroidal))` evaluates the balance quantities on it.

`TrackingRewards` gives the tracking rewards on balance quantities (base height, odometry velocity, capture point, actuated
joint positions): each quantity on the true side and on the reference side and the radial basis function of their difference,
from the tensors of the blocks above.  One HIP launch per refresh (csrc/jm_trackrewards.h) driven by a plan that
jiminy_amd/trackrewards.py builds; specification: tests/golden/ref_tracking_rewards.npz.

`SupportPolygon` gives the projected support polygon (the 2D convex hull of every contact point, at most 16), its barycenter,
the stability margin (the signed distance of the ZMP from its border) and the robustness reward on it, from the `pose` of a
`FrameKinematics` and the `zmp` / `odom_pose` of a `LocomotionQuantities`.  One HIP launch per refresh (csrc/jm_support.h)
driven by a plan that jiminy_amd/support.py builds; specification: tests/golden/ref_support.npz.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

EARTH_SURFACE_GRAVITY = 9.81


class _EngineBlock:
    """What every block bound to an engine repeats: the binding, the tensor check and the mask normalisation.  The
    constructor does nothing: a subclass validates its arguments first and calls `_bind` where it starts to build."""

    def _bind(self, engine) -> None:
        """The engine's topology library, error check and dtype code."""
        import ctypes as C

        from . import _abi
        self._C = C
        self._eng = engine
        self._L = engine._lib.L
        self._check = engine._lib.check
        self._dtype = _abi.JM_F64 if engine.dtype == torch.float64 else _abi.JM_F32

    def _ptr(self, t: Optional[torch.Tensor], dtype=None) -> Optional[int]:
        """The data pointer of a contiguous tensor on the engine's device, of the engine's dtype unless `dtype` names
        another.  None for None and for a tensor without elements (`FootPoseQuantities` with one foot has no relative
        column): the library receives a null pointer, its sign for an absent input or output."""
        if t is None:
            return None
        eng = self._eng
        if not t.is_contiguous() or t.device != eng.device or t.dtype != (dtype or eng.dtype):
            raise ValueError("pipeline block tensors must be contiguous engine-dtype tensors on the engine's device")
        return t.data_ptr() if t.numel() else None

    def _mask(self, lane_mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """A lane mask of any dtype as the contiguous uint8 `[B]` tensor on the engine's device the kernels read."""
        if lane_mask is None:
            return None
        mask = lane_mask.to(device=self._eng.device, dtype=torch.uint8).contiguous()
        if tuple(mask.shape) != (self._eng.batch_size,):
            raise ValueError(f"lane_mask must have shape ({self._eng.batch_size},)")
        return mask

    def _flags(self, t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
        """Per-lane flags a launch reads as they are: bool or uint8 `[B]`, no conversion (a bool tensor is viewed as bytes)."""
        if t is None:
            return None
        if t.dtype == torch.bool:
            t = t.view(torch.uint8)
        B = self._eng.batch_size
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.device != self._eng.device or tuple(t.shape) != (B,):
            raise ValueError(f"{name} must be a contiguous bool or uint8 tensor of shape ({B},) on the engine's device")
        return t


class _PlanBlock(_EngineBlock):
    """A block driven by a plan of the library: `self.plan` (a host plan with `desc()`) is created on the device once by
    `jm_<family>_plan_create` and destroyed with the object by `jm_<family>_plan_destroy` (`_abi.PLAN_FAMILIES`)."""

    def _create_plan(self, family: str) -> None:
        from . import _abi
        C = self._C
        assert family in _abi.PLAN_FAMILIES, family     # (the loader declares the entry points of these families only)
        desc, keep = self.plan.desc()
        self._family, self._plan = family, C.c_void_p()
        with torch.cuda.device(self._eng.device):
            self._check(getattr(self._L, f"jm_{family}_plan_create")(C.byref(desc), C.byref(self._plan)))
        del keep        # (the library copied the description)

    def __del__(self) -> None:
        # (safe on a half-built object -- no `_plan`, or a null one after a failed create -- and never twice)
        plan, self._plan = getattr(self, "_plan", None), None
        if plan:
            try:
                getattr(self._L, f"jm_{self._family}_plan_destroy")(plan)
            except Exception:       # noqa: BLE001  (interpreter shutdown)
                pass


class HipBlocks(_EngineBlock):
    """Per-controller-tick pipeline blocks as single HIP kernel launches (`jm_block_*`).

    Bound to one engine: uses its topology library, device, dtype and launch stream.  All tensors
    are `[rows][B]`-shaped, contiguous, on the engine's device."""

    def __init__(self, engine, encoder_index, command_state_lower, command_state_upper, kp, kd,
                 motors_effort_limit) -> None:
        import numpy as np
        self._bind(engine)

        def host(x, shape):
            a = np.ascontiguousarray(torch.as_tensor(x).detach().cpu().numpy(), dtype=np.float64)
            if a.shape != shape:
                raise ValueError(f"expected an array of shape {shape}, got {a.shape}")
            return a
        M = engine.model.nmotors
        self._M = M
        self._enc = np.ascontiguousarray(torch.as_tensor(encoder_index).cpu().numpy(), dtype=np.int32)
        self._lo, self._hi = host(command_state_lower, (3, M)), host(command_state_upper, (3, M))
        self._kp, self._kd, self._lim = host(kp, (M,)), host(kd, (M,)), host(motors_effort_limit, (M,))

    def pd_controller(self, command_state: torch.Tensor, control_dt: float, out: torch.Tensor) -> None:
        """≙ `pd_controller` (proportional_derivative_controller.py:101-163) on the engine's raw
        encoder field; `command_state` `[3][M][B]` is advanced in place, `out` `[M][B]`."""
        C = self._C
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self._check(self._L.jm_block_pd_controller(
            self._dtype, self._eng.batch_size, self._M, self._ptr(self._eng.field("encoder")),
            self._enc.ctypes.data_as(ip), self._ptr(command_state), self._lo.ctypes.data_as(dp),
            self._hi.ctypes.data_as(dp), self._kp.ctypes.data_as(dp), self._kd.ctypes.data_as(dp),
            self._lim.ctypes.data_as(dp), float(control_dt), self._ptr(out), self._eng._stream()))

    def mahony_filter(self, q: torch.Tensor, omega: torch.Tensor, cf: torch.Tensor, bias_hat: torch.Tensor,
                      kp: float, ki: float, dt: float) -> None:
        """≙ `mahony_filter` (mahony_filter.py:28-101) on the engine's raw IMU field; `q`
        `[4][n_imu][B]`, the others `[3][n_imu][B]`, all updated in place."""
        n_imu = q.shape[1]
        self._check(self._L.jm_block_mahony_filter(
            self._dtype, self._eng.batch_size, n_imu, self._ptr(self._eng.field("imu")), self._ptr(q),
            self._ptr(omega), self._ptr(cf), self._ptr(bias_hat), float(kp), float(ki), float(dt),
            self._eng._stream()))


    def pd_adapter(self, action: torch.Tensor, order: int, command_state: torch.Tensor, is_instantaneous: bool,
                   velocity_deadband, step_dt: float, out: torch.Tensor) -> None:
        """≙ `pd_adapter` (proportional_derivative_controller.py:166-260): `action` `[M][B]` -> target
        acceleration `out` `[M][B]` (command state `[3][M][B]` moved in place when instantaneous)."""
        import numpy as np
        C = self._C
        dp = C.POINTER(C.c_double)
        db = None
        if velocity_deadband is not None:
            db = np.ascontiguousarray(torch.as_tensor(velocity_deadband).cpu().numpy(), dtype=np.float64)
        self._check(self._L.jm_block_pd_adapter(
            self._dtype, self._eng.batch_size, self._M, self._ptr(action), int(order), self._ptr(command_state),
            self._lo.ctypes.data_as(dp), self._hi.ctypes.data_as(dp), int(bool(is_instantaneous)),
            None if db is None else db.ctypes.data_as(dp), float(step_dt), self._ptr(out), self._eng._stream()))

    def motor_safety_limit(self, command: torch.Tensor, kp, kd, soft_position_lower, soft_position_upper,
                           velocity_limit, out: torch.Tensor) -> None:
        """≙ `apply_safety_limits` (blocks/motor_safety_limit.py:20-77) on the engine's raw encoder field."""
        import numpy as np
        C = self._C
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        arr = lambda x: np.ascontiguousarray(np.broadcast_to(np.asarray(torch.as_tensor(x).cpu().numpy(), dtype=np.float64), (self._M,)))  # noqa: E731
        a = [arr(x) for x in (kp, kd, soft_position_lower, soft_position_upper, velocity_limit)]
        self._check(self._L.jm_block_motor_safety_limit(
            self._dtype, self._eng.batch_size, self._M, self._ptr(self._eng.field("encoder")), self._enc.ctypes.data_as(ip),
            self._ptr(command), *[x.ctypes.data_as(dp) for x in a], self._lim.ctypes.data_as(dp), self._ptr(out),
            self._eng._stream()))


class DeformationEstimator(_PlanBlock):
    """≙ `gym_jiminy.common.blocks.DeformationEstimator` (blocks/deformation_estimator.py:416-863), batched: from the
    encoders of the engine and IMU attitude estimates (`[4][n_imu][B]` xyzw in the order of the model's IMU sensors, e.g.
    the state of the Mahony filter) to one deformation quaternion per flexibility point.

    `quat` `[4][n_flex][B]` (the identity until the first `refresh`, :767) and `rpy` `[3][n_flex][B]` (`compute_rpy`) are
    the observation; their columns follow `flexibility_frame_names`, which is NOT the order of `flex_frame_names` but the
    order of the kinematic chains (:613-616).  Deviation from the reference: the compiled model must have a flexibility
    joint at every frame of `flex_frame_names` (`NotImplementedError` otherwise; see jiminy_amd/deformation.py)."""

    def __init__(self, engine, imu_frame_names, flex_frame_names, ignore_twist: bool = True, compute_rpy: bool = True) -> None:
        from . import deformation
        self._bind(engine)
        self.plan = deformation.build_plan(engine.model, imu_frame_names, flex_frame_names, ignore_twist, compute_rpy)
        self.ignore_twist, self.compute_rpy = bool(ignore_twist), bool(compute_rpy)
        self.flexibility_frame_names = list(self.plan.flexibility_frame_names)
        self._n_imu = len(engine.model.sensors["ImuSensor"])
        n_flex, B = self.plan.n_flex, engine.batch_size
        self.quat = torch.zeros((4, n_flex, B), dtype=engine.dtype, device=engine.device)
        self.quat[3] = 1.0
        self.rpy = torch.zeros((3, n_flex, B), dtype=engine.dtype, device=engine.device) if compute_rpy else None
        self._create_plan("deform")

    @property
    def fieldnames(self):
        """≙ `DeformationEstimator.fieldnames` (:819-829)."""
        names = {"quat": [[f"{name}.Quat{e}" for name in self.flexibility_frame_names] for e in ("x", "y", "z", "w")]}
        if self.compute_rpy:
            names["rpy"] = [[".".join((name, e)) for name in self.flexibility_frame_names] for e in ("Roll", "Pitch", "Yaw")]
        return names

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """The identity (and zero angles) on the masked lanes, by selection; on every lane without a mask."""
        unit = torch.zeros_like(self.quat)
        unit[3] = 1.0
        if lane_mask is None:
            self.quat.copy_(unit)
            if self.rpy is not None:
                self.rpy.zero_()
        else:
            m = lane_mask[None, None, :]
            self.quat.copy_(torch.where(m, unit, self.quat))
            if self.rpy is not None:
                self.rpy.copy_(torch.where(m, torch.zeros_like(self.rpy), self.rpy))

    def refresh(self, imu_quat: torch.Tensor) -> None:
        """≙ `refresh_observation` (:831-863): one launch on the engine's stream; no allocation, copy or synchronisation."""
        eng = self._eng
        if tuple(imu_quat.shape) != (4, self._n_imu, eng.batch_size):
            raise ValueError(f"imu_quat must have shape (4, {self._n_imu}, {eng.batch_size})")
        self._check(self._L.jm_block_deformation_estimator(
            self._plan, self._dtype, eng.batch_size, self._ptr(eng.field("encoder")), self._ptr(imu_quat),
            self._ptr(self.quat), self._ptr(self.rpy), eng._stream()))


class MahonyFilter(_PlanBlock):
    """≙ `gym_jiminy.common.blocks.MahonyFilter` (blocks/mahony_filter.py:104-393), batched over the IMU sensors of the
    engine's model (sensor order) and its lanes.

    Observation: `quat` `[4][n_imu][B]` (xyzw), `omega` `[3][n_imu][B]`, `rpy` `[3][n_imu][B]` (`compute_rpy`, else None);
    state: `bias` `[3][n_imu][B]`.  `reset(lane_mask)` is the first refresh of an episode (:340-374: the true orientation
    of the IMU frames with `exact_init`, else from the accelerometers) and reads the engine's `q` and IMU rows: call it
    after the engine's `start` / `reset_lanes`.  `refresh(dt)` is every later one (:376-393).  One launch each."""

    def __init__(self, engine, *, ignore_twist: bool = False, exact_init: bool = True, kp=1.0, ki=0.1,
                 compute_rpy: bool = False) -> None:
        from . import attitude
        self._bind(engine)
        self.plan = attitude.build_plan(engine.model, kp, ki)
        self.ignore_twist, self.exact_init, self.compute_rpy = bool(ignore_twist), bool(exact_init), bool(compute_rpy)
        self.kp, self.ki = self.plan.kp, self.plan.ki
        n_imu, B = self.plan.n_imu, engine.batch_size
        new = lambda rows: torch.zeros((rows, n_imu, B), dtype=engine.dtype, device=engine.device)      # noqa: E731
        self.quat, self.omega, self.bias, self._cf = new(4), new(3), new(3), new(3)
        self.quat[3] = 1.0      # (:286)
        self.rpy = new(3) if compute_rpy else None
        self._twist_of = None   # the `twist` state of a BodyObserver behind this filter: zeroed by the same launch
        self._create_plan("attitude")

    @property
    def fieldnames(self):
        """≙ `MahonyFilter.fieldnames` (:321-335)."""
        imu = self.plan.imu_names
        names = {"quat": [[f"{n}.Quat{e}" for n in imu] for e in ("X", "Y", "Z", "W")],
                 "omega": [[f"{n}.{e}" for n in imu] for e in ("X", "Y", "Z")]}
        if self.compute_rpy:
            names["rpy"] = [[f"{n}.{e}" for n in imu] for e in ("Roll", "Pitch", "Yaw")]
        return names

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        eng, ptr = self._eng, self._ptr
        mask = self._mask(lane_mask)
        twist = None if self._twist_of is None else self._twist_of.twist
        self._check(self._L.jm_block_attitude_init(
            self._plan, self._dtype, eng.batch_size, ptr(eng.field("q")), ptr(eng.field("imu")), ptr(mask, torch.uint8),
            int(self.exact_init), ptr(self.quat), ptr(self.omega), ptr(self._cf), ptr(self.bias), ptr(twist), ptr(self.rpy),
            eng._stream()))

    def refresh(self, dt: float) -> None:
        eng, ptr = self._eng, self._ptr
        if not dt > 0.0:
            raise ValueError("This block does not support time-continuous update.")     # (:288-291)
        self._check(self._L.jm_block_mahony_observer(
            self._plan, self._dtype, eng.batch_size, ptr(eng.field("imu")), ptr(self.quat), ptr(self.omega),
            ptr(self._cf), ptr(self.bias), float(dt), int(self.ignore_twist), ptr(self.rpy), eng._stream()))


class BodyObserver:
    """≙ `gym_jiminy.common.blocks.BodyObserver` (blocks/body_orientation_observer.py:74-266) behind a `MahonyFilter`:
    orientation `quat` `[4][n_imu][B]`, angular velocity `omega` `[3][n_imu][B]` and `rpy` (`compute_rpy`, else None) of
    the parent body of every IMU.  `twist_time_constant`: None keeps the filter's twist, 0 removes it, > 0 removes it and
    estimates it with a leaky integrator (state `twist` `[n_imu][B]`)."""

    def __init__(self, engine, mahony: MahonyFilter, *, twist_time_constant: Optional[float] = None,
                 compute_rpy: bool = True) -> None:
        from . import attitude
        if mahony._eng is not engine:
            raise ValueError("the Mahony filter belongs to another engine")
        self._eng, self._mahony = engine, mahony
        self.compute_rpy = bool(compute_rpy)
        # (:129-140)
        if twist_time_constant is None:
            self.twist_time_constant_inv, self._mode = None, attitude.TWIST_KEEP
        elif twist_time_constant > 0.0:
            self.twist_time_constant_inv, self._mode = 1.0 / float(twist_time_constant), attitude.TWIST_INTEGRATE
        else:
            self.twist_time_constant_inv, self._mode = float("inf"), attitude.TWIST_REMOVE
        n_imu, B = mahony.plan.n_imu, engine.batch_size
        new = lambda rows: torch.zeros((rows, n_imu, B), dtype=engine.dtype, device=engine.device)      # noqa: E731
        self.quat, self.omega = new(4), new(3)
        self.quat[3] = 1.0      # (:219)
        self.rpy = new(3) if compute_rpy else None
        self.twist = torch.zeros((n_imu, B), dtype=engine.dtype, device=engine.device)
        mahony._twist_of = self
        self._scratch = None

    @property
    def fieldnames(self):
        """≙ `BodyObserver.fieldnames` (:221-235)."""
        imu = self._mahony.plan.imu_names
        names = {"quat": [[f"{n}.Quat{e}" for n in imu] for e in ("X", "Y", "Z", "W")]}
        if self.compute_rpy:
            names["rpy"] = [[f"{n}.{e}" for n in imu] for e in ("Roll", "Pitch", "Yaw")]
        names["omega"] = [[f"{n}.{e}" for n in imu] for e in ("X", "Y", "Z")]
        return names

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """The first refresh of an episode on the masked lanes: the reference refreshes every observer once at reset,
        behind the filter's initialisation, with a zero twist estimate and a zero angular velocity (:211-219, :237-266) --
        the twist, if any, is removed and nothing is integrated.  Call it after the filter's `reset`, which zeroes the twist
        state of those lanes.  The other lanes keep their observation bit for bit (selection, not arithmetic)."""
        if lane_mask is None:
            self._launch(0.0, False, self.quat, self.omega, self.rpy)
            return
        mask = lane_mask.to(device=self._eng.device, dtype=torch.bool)      # (any mask dtype, as `MahonyFilter.reset` takes)
        if tuple(mask.shape) != (self._eng.batch_size,):
            raise ValueError(f"lane_mask must have shape ({self._eng.batch_size},)")
        if self._scratch is None:
            self._scratch = (torch.empty_like(self.quat), torch.empty_like(self.omega),
                             None if self.rpy is None else torch.empty_like(self.rpy))
        self._launch(0.0, False, *self._scratch)
        m = mask[None, None, :]
        for mine, fresh in zip((self.quat, self.omega, self.rpy), self._scratch):
            if mine is not None:
                mine.copy_(torch.where(m, fresh, mine))

    def refresh(self, dt: float) -> None:
        """≙ `refresh_observation` (:237-266): one launch on the engine's stream."""
        self._launch(dt, True, self.quat, self.omega, self.rpy)

    def _launch(self, dt: float, integrate: bool, quat, omega, rpy) -> None:
        from . import attitude
        eng, m = self._eng, self._mahony
        mode = self._mode if integrate or self._mode != attitude.TWIST_INTEGRATE else attitude.TWIST_REMOVE
        tci = self.twist_time_constant_inv if mode == attitude.TWIST_INTEGRATE else 0.0
        m._check(m._L.jm_block_body_observer(
            m._plan, m._dtype, eng.batch_size, m._ptr(m.quat), m._ptr(m.omega), m._ptr(quat), m._ptr(omega),
            m._ptr(self.twist), int(mode), float(tci), float(dt), m._ptr(rpy), eng._stream()))


def frame_fieldnames(frame_names, compute_rpy: bool, compute_velocity: bool, average: bool):
    """Names of the rows of the tensors of a `FrameKinematics` block, `[row][frame]` per tensor."""
    fr = list(frame_names)
    pose = ("X", "Y", "Z", "QuatX", "QuatY", "QuatZ", "QuatW")
    spatial = ("LinX", "LinY", "LinZ", "AngX", "AngY", "AngZ")
    names = {"pose": [[f"{n}.{e}" for n in fr] for e in pose]}
    if compute_rpy:
        names["rpy"] = [[f"{n}.{e}" for n in fr] for e in ("Roll", "Pitch", "Yaw")]
    if compute_velocity:
        names["velocity"] = [[f"{n}.{e}" for n in fr] for e in spatial]
    if average:
        names["average_velocity"] = [[f"{n}.{e}" for n in fr] for e in spatial]
        names["pose_mean"] = [[f"{n}.{e}" for n in fr] for e in pose]
        names["quat_no_yaw"] = [[f"{n}.Quat{e}" for n in fr] for e in ("X", "Y", "Z", "W")]
    return names


class FrameKinematics(_PlanBlock):
    """Pose and velocity of named frames of the engine's model, per lane, and their average over an environment step.

    ≙ `FramePosition` / `FrameOrientation` / `FrameXYZQuat` (quantities/generic.py:298-950) for `pose` `[7][K][B]` (x y z,
    quaternion xyzw) and `rpy` `[3][K][B]` (`compute_rpy`, else None), pinocchio's `getFrameVelocity` for `velocity`
    `[6][K][B]` (linear, angular; `compute_velocity`, else None) in the reference frame of every frame (`reference_frames`:
    "LOCAL" (default), "LOCAL_WORLD_ALIGNED" or, with `average`, "ODOMETRY", whose instantaneous velocity is LOCAL).
    With `average`: `average_velocity` `[6][K][B]` ≙ `FrameSpatialAverageVelocity` (:1429-1534) and, for ODOMETRY frames,
    `BaseSpatialAverageVelocity` (quantities/locomotion.py:222-288); `pose_mean` `[7][K][B]` ≙ `AverageFrameXYZQuat`
    (:1289-1360); `quat_no_yaw` `[4][K][B]` ≙ `AverageFrameRollPitch` (:1363-1426).

    `state=(q, v)`: `[rows][B]` tensors read instead of the engine's `q`, `v` (the state of a reference trajectory,
    `ReferenceTrajectory.q` / `.v`), without the per-lane joint placements: the reference evaluates a trajectory on the
    trajectory's own robot.

    `reset(lane_mask)` evaluates the frames at the state the engine's `start` / `reset_lanes` wrote and makes it the previous
    pose of the average; `refresh()` evaluates them at the engine's current `q`, `v` (with the per-lane joint placements when
    the engine has a biased model bound); `refresh_average(step_dt)` averages between the pose of the previous call (or
    reset) and the current `pose`.  One launch each, no allocation, copy or synchronisation; the tensors never change
    identity."""

    def __init__(self, engine, frame_names, *, reference_frames=None, compute_rpy: bool = False, compute_velocity: bool = True,
                 average: bool = False, state=None) -> None:
        from . import frames
        # `state`: a pair (q, v) of `[rows][B]` tensors read instead of the engine's fields (v may be None without
        # `compute_velocity`) -- the state of a reference trajectory, which the reference evaluates on the trajectory's own
        # robot, not on the per-episode biased model: the lane's joint placements are not applied then
        self._state = None
        if state is not None:
            q, v = state
            if tuple(q.shape) != (engine.model.nq, engine.batch_size):
                raise ValueError(f"state q must have shape ({engine.model.nq}, {engine.batch_size})")
            if v is not None and tuple(v.shape) != (engine.model.nv, engine.batch_size):
                raise ValueError(f"state v must have shape ({engine.model.nv}, {engine.batch_size})")
            if v is None and compute_velocity:
                raise ValueError("the frame velocity needs v: give state=(q, v) or compute_velocity=False")
            self._state = (q, v)
        self._bind(engine)
        self.plan = frames.build_plan(engine.model, frame_names, reference_frames)
        self.frame_names = list(self.plan.frame_names)
        self.compute_rpy, self.compute_velocity, self.average = bool(compute_rpy), bool(compute_velocity), bool(average)
        if not self.average and frames.ODOMETRY in self.plan.modes:
            raise NotImplementedError("the ODOMETRY reference frame is defined for the step average only: pass average=True")
        K, B = self.plan.n_frames, engine.batch_size
        new = lambda rows: torch.zeros((rows, K, B), dtype=engine.dtype, device=engine.device)      # noqa: E731
        self.pose = new(7)
        self.pose[6] = 1.0
        self.rpy = new(3) if self.compute_rpy else None
        self.velocity = new(6) if self.compute_velocity else None
        self.average_velocity = self.pose_mean = self.quat_no_yaw = self.pose_prev = None
        if self.average:
            self.average_velocity, self.pose_mean, self.quat_no_yaw, self.pose_prev = new(6), new(7), new(4), new(7)
            for t in (self.pose_mean[6], self.quat_no_yaw[3], self.pose_prev[6]):
                t.fill_(1.0)
        self._create_plan("frames")

    def index(self, frame_name: str) -> int:
        """Column of a frame in the tensors."""
        return self.frame_names.index(frame_name)

    @property
    def fieldnames(self):
        return frame_fieldnames(self.frame_names, self.compute_rpy, self.compute_velocity, self.average)

    def _kinematics(self, mask: Optional[torch.Tensor], pose_prev: Optional[torch.Tensor]) -> None:
        eng, ptr = self._eng, self._ptr
        if self._state is not None:
            q, v, model_lane = self._state[0], self._state[1], None
        else:
            q, v, model_lane = eng.field("q"), eng.field("v"), eng._fields.get("model_lane")
        self._check(self._L.jm_block_frame_kinematics(
            self._plan, self._dtype, eng.batch_size, ptr(q), ptr(v) if self.compute_velocity else None, ptr(model_lane),
            ptr(mask, torch.uint8), ptr(self.pose), ptr(pose_prev), ptr(self.rpy), ptr(self.velocity), eng._stream()))

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """The frames at the state of a new episode on the masked lanes (every lane without a mask), which also becomes
        the previous pose of their step average.  The other lanes keep every tensor bit for bit.  Call it after the
        engine's `start` / `reset_lanes`."""
        self._kinematics(self._mask(lane_mask), self.pose_prev)

    def refresh(self) -> None:
        """One launch on the engine's stream: `pose`, `rpy`, `velocity` at the engine's `q`, `v`."""
        self._kinematics(None, None)

    def refresh_average(self, step_dt: float) -> None:
        """One launch: `average_velocity`, `pose_mean`, `quat_no_yaw` between the previous pose and `pose`, which then
        becomes the previous one."""
        if not self.average:
            raise RuntimeError("this block was built without average=True")
        if not step_dt > 0.0:
            raise ValueError("the step average needs a positive step_dt")
        eng, ptr = self._eng, self._ptr
        self._check(self._L.jm_block_frame_average(
            self._plan, self._dtype, eng.batch_size, ptr(self.pose_prev), ptr(self.pose), 1.0 / float(step_dt),
            ptr(self.average_velocity), ptr(self.pose_mean), ptr(self.quat_no_yaw), eng._stream()))


class CentroidalState(_PlanBlock):
    """The centroidal quantities of a state other than the engine's own: `centroidal` `[15][B]` in the row layout of the
    engine's `centroidal` field -- com (3), hg (6: linear then angular, about the centre of mass, world axes), dhg (6) -- from
    `state=(q, v, a)`, `[rows][B]` tensors in pinocchio's convention (`ReferenceTrajectory.q` / `.v` / `.a`); `a` may be None:
    the dhg rows stay zero.  ≙ `pin.computeCentroidalMomentumTimeVariation` on the state of a trajectory
    (jiminy_py/dynamics.py:496-499, reached from `StateQuantity.refresh`, bases/quantities.py:1494-1518): dhg holds no gravity
    and no external force.  The model is the nominal one, never the lane's biased one: the reference evaluates a trajectory on
    the trajectory's own robot.  The centre-of-mass velocity is `centroidal[3:6] / mass`.

    `refresh()` evaluates every lane, `reset(lane_mask)` the masked ones (every lane without a mask) and keeps the others bit
    for bit.  Each is one launch on the engine's stream, without allocation, copy or synchronisation; the tensor never changes
    identity."""

    def __init__(self, engine, state) -> None:
        import os

        from . import centroidal
        if os.environ.get("JIMINY_AMD_TENSOR_BLOCKS", "0") == "1":
            raise NotImplementedError("the centroidal state has no tensor-program form (JIMINY_AMD_TENSOR_BLOCKS=1): "
                                      "the evaluation exists as the HIP kernel only")
        q, v, a = state
        model, B = engine.model, engine.batch_size
        for name, t, rows in (("q", q, model.nq), ("v", v, model.nv), ("a", a, model.nv)):
            if t is None and name == "a":
                continue
            if t is None or tuple(t.shape) != (rows, B):
                raise ValueError(f"state {name} must have shape ({rows}, {B})")
        self._bind(engine)
        self._state = (q, v, a)
        self.plan = centroidal.build_plan(model)
        self.mass = self.plan.mass
        self.has_acceleration = a is not None
        self.centroidal = torch.zeros((centroidal.ROWS, B), dtype=engine.dtype, device=engine.device)
        self._create_plan("centroidal")

    @property
    def fieldnames(self):
        xyz = ("X", "Y", "Z")
        return {"centroidal": [f"Com.{e}" for e in xyz] + [f"{h}.{k}{e}" for h in ("Momentum", "MomentumRate") for k in ("Lin", "Ang")
                                                             for e in xyz]}

    def _launch(self, mask: Optional[torch.Tensor]) -> None:
        eng, ptr = self._eng, self._ptr
        q, v, a = self._state
        self._check(self._L.jm_block_centroidal_state(
            self._plan, self._dtype, eng.batch_size, ptr(q), ptr(v), ptr(a), ptr(mask, torch.uint8), ptr(self.centroidal),
            eng._stream()))

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """The quantities at the state tensors on the masked lanes (every lane without a mask); the other lanes keep every
        bit."""
        self._launch(self._mask(lane_mask))

    def refresh(self) -> None:
        """One launch on the engine's stream: `centroidal` at the state tensors."""
        self._launch(None)


LOCOMOTION_SCALARS = ("force_vertical_max", "ground_distance_min", "reward_momentum", "reward_friction")


def locomotion_fieldnames(contact_names, foot_frame_names, momentum: bool, forces: bool, ground_profile: bool = False):
    """Names of the rows of the tensors of a `LocomotionQuantities` block."""
    xyz = ("X", "Y", "Z")
    names = {"com": [f"Com.{e}" for e in xyz], "vcom": [f"ComVelocity.{e}" for e in xyz],
             "odom_pose": ["Odom.X", "Odom.Y", "Odom.Yaw"], "zmp": ["Zmp.X", "Zmp.Y"], "dcm": ["Dcm.X", "Dcm.Y"],
             "scalars": list(LOCOMOTION_SCALARS)}
    if momentum:
        names["h_angular"] = [f"BaseMomentum.Ang{e}" for e in xyz]
    if forces:
        names["contact_force_rel"] = [[f"{n}.{e}" for n in contact_names] for e in ("LinX", "LinY", "LinZ", "AngX", "AngY", "AngZ")]
        names["foot_force_vertical"] = [f"{n}.ForceVertical" for n in foot_frame_names]
    if ground_profile:
        names["contact_ground"] = [[f"{n}.{e}" for n in contact_names] for e in ("GroundHeight", "NormalX", "NormalY", "NormalZ")]
    return names


class LocomotionQuantities(_PlanBlock):
    """The balance quantities of the reference's locomotion layer (quantities/locomotion.py, compositions/locomotion.py) per
    lane, from what a step left on the device: `com`, `vcom` `[3][B]` ≙ `CenterOfMass` (:814-887); `odom_pose` `[3][B]` ≙
    `BaseOdometryPose` (:158-219); `zmp` `[2][B]` ≙ `ZeroMomentPoint` (:914-1017; NaN in free fall); `dcm` `[2][B]` ≙
    `CapturePoint` (:1021-1124); `h_angular` `[3][B]` ≙ `AverageBaseMomentum` (:344-412; `momentum`, else None);
    `contact_force_rel` `[6][n_contacts][B]` ≙ `MultiContactNormalizedSpatialForce` (:1128-1268) and `foot_force_vertical`
    `[n_feet][B]` ≙ `MultiFootNormalizedForceVertical` (:1272-1481) on flat ground (`forces`, else None); `scalars` `[4][B]`,
    rows `LOCOMOTION_SCALARS`: the largest normalised vertical contact force (`ImpactForceTermination`), the height of the lowest
    contact frame (`FlyingTermination`), and `MinimizeAngularMomentumReward` / `MinimizeFrictionReward` with `momentum_cutoff` /
    `friction_cutoff` (None: that row stays zero).

    `frames`: the `FrameKinematics` block of the same engine, holding 'root_joint' (LOCAL) and every contact frame, with
    `average=True` unless `momentum=False`; refresh it first.  The force quantities need the constraint contact model
    (`forces=False` leaves them out).  `refresh()` is one launch on the engine's stream, without allocation, copy or
    synchronisation; `reset(lane_mask)` evaluates the masked lanes (every lane without a mask) at the state the engine's
    `start` / `reset_lanes` wrote and keeps the others bit for bit.  The tensors never change identity.

    `state=(q, centroidal)`: the quantities of another state than the engine's -- `QuantityEvalMode.REFERENCE`.  `q` `[nq][B]`
    (`ReferenceTrajectory.q`) and `centroidal`, a `CentroidalState` block of that state or its `[15][B]` tensor, are read
    instead of the engine's fields; `frames` must be a `FrameKinematics(state=...)` block of the same state; the lane's biased
    model is not applied.  A recorded trajectory carries no constraint multipliers: `forces=True` raises.  Where the state has
    no acceleration (`CentroidalState` built with `a` None), `zmp` is None: the reference's `ZeroMomentPoint.initialize` raises
    in that case.

    `ground_profile=True`: height-map ground with the constraint contact model, whose contact rows live in the local frame
    [t0 t1 n] of the surface under each contact point (`FrameConstraint::setNormal`).  Every `refresh()` / `reset()` reads the
    engine's current height map, its grid and its `ground_offset` field (`set_ground_heightmap`, `set_ground_offsets`; they may
    be bound after the block is built and change between launches) and queries the ground under every contact point at the
    lane's offset: `foot_force_vertical` is then the world vertical force, the third row of [t0 t1 n] on the multipliers of
    every contact, and `ground_distance_min` the minimum of `(z - height) * normal_z` (`_MultiContactMinGroundDistance`,
    compositions/locomotion.py:449-540).  `contact_ground` `[4][n_contacts][B]` holds the height and the unit normal under
    every contact point (None without the option).  `contact_force_rel`, `force_vertical_max` and the friction reward stay in
    the local contact frame, as in the reference; the other quantities do not look at the ground.  With no map bound the
    results are the flat ones.  Not with `state=`: the reference evaluates the ground distance in TRUE mode only.
    Without the option the block refuses an engine that has a height map bound when the block is built; a map bound LATER
    (`WalkerVecEnv` binds its `ground_profile` in `reset()`) is not seen, and the flat formulas are then evaluated on it."""

    def __init__(self, engine, frames: "FrameKinematics", *, foot_frame_names="auto", zmp_reference_frame="LOCAL",
                 dcm_reference_frame="LOCAL", momentum_cutoff: Optional[float] = None, friction_cutoff: Optional[float] = None,
                 momentum: bool = True, forces: bool = True, state=None, ground_profile: bool = False) -> None:
        from . import _abi, locomotion
        from . import frames as frames_
        model = engine.model
        if not model.has_freeflyer:
            raise ValueError("Only legged robot with floating base are supported: the model has no free-flyer.")
        self._state, has_acceleration = None, True
        self.ground_profile = bool(ground_profile)
        if self.ground_profile and state is not None:
            raise NotImplementedError("ground_profile=True with a reference state: the reference evaluates the distance to the "
                                      "ground in TRUE mode only (`_MultiContactMinGroundDistance`)")
        if state is not None:
            if forces:
                raise NotImplementedError("the contact force quantities of a reference state: a recorded trajectory carries no "
                                          "constraint multipliers (`State.lambda_c`); pass forces=False")
            q, centroidal = state
            if isinstance(centroidal, CentroidalState):
                has_acceleration, centroidal = centroidal.has_acceleration, centroidal.centroidal
            if tuple(q.shape) != (model.nq, engine.batch_size):
                raise ValueError(f"state q must have shape ({model.nq}, {engine.batch_size})")
            if tuple(centroidal.shape) != (15, engine.batch_size):
                raise ValueError(f"state centroidal must have shape (15, {engine.batch_size})")
            if frames._state is None or frames._state[0] is not q:
                raise ValueError("the frame kinematics block must be built on the same state: FrameKinematics(state=(q, v))")
            self._state = (q, centroidal)
        if state is None and "centroidal" not in engine._fields:
            raise ValueError("the locomotion quantities read the 'centroidal' output of the engine: build it with "
                             "extra_outputs=(..., 'centroidal') or call enable_output('centroidal')")
        if frames._eng is not engine:
            raise ValueError("the frame kinematics block belongs to another engine")
        for cutoff in (momentum_cutoff, friction_cutoff):
            if cutoff is not None and not float(cutoff) > 0.0:
                raise ValueError("a reward cutoff must be positive")
        constraint_model = engine._options["contacts"]["model"] == "constraint"
        self.momentum, self.forces = bool(momentum), bool(forces)
        if (momentum_cutoff is not None and not self.momentum) or (friction_cutoff is not None and not self.forces):
            raise ValueError("a reward cutoff was given for a quantity that is switched off")
        if self.momentum and not frames.average:
            raise ValueError("the angular momentum reads the step average of the root frame: build the frame kinematics "
                             "block with average=True (or pass momentum=False)")
        if self.forces and not constraint_model:
            raise NotImplementedError("the contact force quantities read the multipliers of the contact constraints "
                                      "(`lambda_c`): contacts.model = 'spring_damper' has none (pass forces=False for the "
                                      "other quantities)")
        if engine._ground is not None and not self.ground_profile:
            raise NotImplementedError("the locomotion quantities assume flat ground: on a height map the local contact frame "
                                      "is the surface's (pass ground_profile=True)")
        self.plan = locomotion.build_plan(model, frames.frame_names, foot_frame_names=foot_frame_names,
                                          zmp_reference_frame=zmp_reference_frame, dcm_reference_frame=dcm_reference_frame)
        if self.momentum and frames.plan.modes[frames.index("root_joint")] != frames_.LOCAL:
            raise ValueError("the angular momentum reads the LOCAL step-average velocity of 'root_joint': the frame kinematics "
                             "block holds it in another reference frame")
        self._bind(engine)
        self._frames = frames
        self.foot_frame_names = list(self.plan.foot_frame_names)
        self.momentum_cutoff = None if momentum_cutoff is None else float(momentum_cutoff)
        self.friction_cutoff = None if friction_cutoff is None else float(friction_cutoff)
        B, nc = engine.batch_size, self.plan.n_contacts
        new = lambda *shape: torch.zeros((*shape, B), dtype=engine.dtype, device=engine.device)      # noqa: E731
        self.com, self.vcom, self.odom_pose, self.zmp, self.dcm, self.scalars = new(3), new(3), new(3), new(2), new(2), new(4)
        if not has_acceleration:
            self.zmp = None
        self.h_angular = new(3) if self.momentum else None
        self.contact_force_rel = new(6, nc) if self.forces else None
        self.foot_force_vertical = new(self.plan.n_feet) if self.forces else None
        self.contact_ground = new(4, nc) if self.ground_profile else None
        self._ground_io = _abi.LocomotionGround() if self.ground_profile else None
        rows = _abi.constraint_rows(model)
        self._flag_row, self._lambda_row = rows["n_bounds"], 2 * rows["n_bounds"]
        self._q_row = int(model.idx_q[1])
        self._io = _abi.LocomotionIO()
        self._create_plan("locomotion")

    @property
    def fieldnames(self):
        return locomotion_fieldnames(self._eng.model.contacts, self.foot_frame_names, self.momentum, self.forces, self.ground_profile)

    @property
    def force_vertical_max(self) -> torch.Tensor:
        return self.scalars[0]

    @property
    def ground_distance_min(self) -> torch.Tensor:
        return self.scalars[1]

    @property
    def reward_momentum(self) -> torch.Tensor:
        return self.scalars[2]

    @property
    def reward_friction(self) -> torch.Tensor:
        return self.scalars[3]

    def _launch(self, mask: Optional[torch.Tensor]) -> None:
        eng, fr, io, ptr = self._eng, self._frames, self._io, self._ptr
        if self._state is not None:
            q, centroidal = self._state
            io.centroidal, io.q_root, io.model_lane = ptr(centroidal), ptr(q[self._q_row:self._q_row + 7]), None
        else:
            io.centroidal, io.q_root = ptr(eng.field("centroidal")), ptr(eng.field("q")[self._q_row:self._q_row + 7])
            io.model_lane = ptr(eng._fields.get("model_lane"))
        io.con_lambda = io.con_flags = None
        if self.forces:
            # (the constraint state of the engine exists once the constraint contact model is selected)
            flags, data = eng._fields["con_flags"], eng._fields["con_data"]
            nc = self.plan.n_contacts
            io.con_flags = ptr(flags[self._flag_row:self._flag_row + nc], torch.int32)
            io.con_lambda = ptr(data[self._lambda_row:self._lambda_row + 4 * nc])
        io.v_avg = ptr(fr.average_velocity) if self.momentum else None
        io.quat_no_yaw = ptr(fr.quat_no_yaw) if self.momentum else None
        io.pose = ptr(fr.pose)
        io.lane_mask = ptr(mask, torch.uint8)
        for name in ("com", "vcom", "odom_pose", "zmp", "dcm", "h_angular", "contact_force_rel", "foot_force_vertical", "scalars"):
            setattr(io, name, ptr(getattr(self, name)))
        if not self.ground_profile:
            self._check(self._L.jm_block_locomotion(self._plan, self._dtype, eng.batch_size, self._C.byref(io),
                                                    self.momentum_cutoff or 0.0, self.friction_cutoff or 0.0, eng._stream()))
            return
        # the engine's height map, grid and offsets as they are bound now
        g, heights = self._ground_io, eng._ground
        g.heights, g.offsets, g.contact_ground = ptr(heights), None, ptr(self.contact_ground)
        if heights is not None:
            g.ny, g.nx = int(heights.shape[0]), int(heights.shape[1])
            g.x0, g.y0, g.dx, g.dy = eng._ground_grid
            g.offsets = ptr(eng._fields.get("ground_offset"))
        self._check(self._L.jm_block_locomotion_ground(self._plan, self._dtype, eng.batch_size, self._C.byref(io), self._C.byref(g),
                                                       self.momentum_cutoff or 0.0, self.friction_cutoff or 0.0, eng._stream()))

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """The quantities at the state of a new episode on the masked lanes (every lane without a mask); the other lanes
        keep every tensor bit for bit.  Call it after the engine's `start` / `reset_lanes` and the reset of `frames`."""
        self._launch(self._mask(lane_mask))

    def refresh(self) -> None:
        """One launch on the engine's stream, behind the refresh (and the step average) of `frames`."""
        self._launch(None)


ACTUATION_SCALARS = ("power", "power_average", "reward_power")


def actuation_fieldnames(motor_names):
    """Names of the rows of the tensors of an `ActuatedJointQuantities` block."""
    names = {k: [f"{n}.{label}" for n in motor_names]
             for k, label in (("position", "Position"), ("velocity", "Velocity"), ("acceleration", "Acceleration"),
                              ("bound_low", "BoundLow"), ("bound_high", "BoundHigh"))}
    names["scalars"] = list(ACTUATION_SCALARS)
    return names


class ActuatedJointQuantities(_PlanBlock):
    """The actuated-joint part of the reference's quantity layer (quantities/generic.py:1538-1887, compositions/generic.py:
    153-191, 456-661) per lane, from the engine's `q / v / a / command`, each tensor in motor order: `position`, `velocity`,
    `acceleration` `[M][B]` ≙ `MultiActuatedJointKinematic` (:1538-1691; `motor_side`: all three times the mechanical reduction);
    `bound_low`, `bound_high` `[M][B]` ≙ `_MultiActuatedJointBoundDistance` (compositions/generic.py:456-502; always joint side);
    `safety` `[B]` int32: the number of motors inside `position_margin` of a stop and approaching it faster than `velocity_max`
    (`MechanicalSafetyTermination`, :505-595; both None: not evaluated); `scalars` `[3][B]`, rows `ACTUATION_SCALARS`: the
    mechanical power ≙ `MechanicalPowerConsumption` in `generator_mode` (quantities/generic.py:1694-1812), its average over the
    last `power_horizon` seconds of environment steps ≙ `AverageMechanicalPowerConsumption` (:1819-1887; None: no window, the
    row stays zero and `power_average` raises), and `MinimizeMechanicalPowerConsumption` with `power_cutoff` on that average
    (compositions/generic.py:153-191; None: the row stays zero).

    The window is state of the block: `power_ring` `[max_stack][B]` and `power_count` `[B]`, the number of pushes of every lane
    since its restart.  `reset(lane_mask)` restarts the windows of the masked lanes (every lane without a mask) at the state
    the engine's `start` / `reset_lanes` wrote and keeps the other lanes bit for bit; `refresh()` pushes one environment step:
    call it once per step.  Both are one launch on the engine's stream, without allocation, copy or synchronisation, and no
    launch argument changes from step to step.  The tensors never change identity.  One window per block: a reward and a
    termination on different horizons take two blocks."""

    def __init__(self, engine, *, generator_mode="CHARGE", power_horizon: Optional[float] = None,
                 power_cutoff: Optional[float] = None, position_margin: Optional[float] = None,
                 velocity_max: Optional[float] = None, motor_side: bool = False, step_dt: Optional[float] = None) -> None:
        from . import _abi, actuation
        if power_cutoff is not None and not float(power_cutoff) > 0.0:
            raise ValueError("a reward cutoff must be positive")
        if power_cutoff is not None and power_horizon is None:
            raise ValueError("power_cutoff rewards the average power: give power_horizon as well")
        if (position_margin is None) != (velocity_max is None):
            raise ValueError("the mechanical-safety count needs position_margin and velocity_max together")
        if velocity_max is not None and (not float(velocity_max) >= 0.0 or not float(position_margin) >= 0.0):
            raise ValueError("position_margin and velocity_max must not be negative")
        self.plan = actuation.build_plan(engine.model, generator_mode=generator_mode, power_horizon=power_horizon, step_dt=step_dt)
        self._bind(engine)
        self.motor_side = bool(motor_side)
        self.power_cutoff = None if power_cutoff is None else float(power_cutoff)
        self.position_margin = None if position_margin is None else float(position_margin)
        self.velocity_max = None if velocity_max is None else float(velocity_max)
        B, M = engine.batch_size, self.plan.n_motors
        new = lambda *shape, dtype=engine.dtype: torch.zeros((*shape, B), dtype=dtype, device=engine.device)      # noqa: E731
        self.position, self.velocity, self.acceleration, self.bound_low, self.bound_high = (new(M) for _ in range(5))
        self.scalars, self.safety = new(3), new(dtype=torch.int32)
        self.power_ring, self.power_count = new(self.plan.max_stack), new(dtype=torch.int32)
        self._io = _abi.ActuationIO()
        self._create_plan("actuation")

    @property
    def fieldnames(self):
        return actuation_fieldnames(self.plan.motor_names)

    @property
    def power(self) -> torch.Tensor:
        return self.scalars[0]

    @property
    def power_average(self) -> torch.Tensor:
        if not self.plan.has_horizon:
            raise ValueError("the block has no window: build it with power_horizon")
        return self.scalars[1]

    @property
    def reward_power(self) -> torch.Tensor:
        if self.power_cutoff is None:
            raise ValueError("the block has no reward: build it with power_cutoff")
        return self.scalars[2]

    def _launch(self, mode: int, mask: Optional[torch.Tensor]) -> None:
        eng, io, ptr = self._eng, self._io, self._ptr
        for name in ("q", "v", "a", "command"):
            setattr(io, name, ptr(eng.field(name)))
        io.lane_mask = ptr(mask, torch.uint8)
        for name in ("position", "velocity", "acceleration", "bound_low", "bound_high", "scalars"):
            setattr(io, name, ptr(getattr(self, name)))
        io.safety = ptr(self.safety, torch.int32) if self.velocity_max is not None else None
        # (without a horizon the window is not run: rows 1-2 of `scalars` stay zero)
        io.power_ring = ptr(self.power_ring) if self.plan.has_horizon else None
        io.power_count = ptr(self.power_count, torch.int32) if self.plan.has_horizon else None
        self._check(self._L.jm_block_actuation(
            self._plan, self._dtype, eng.batch_size, self._C.byref(io), mode, int(self.motor_side),
            self.position_margin if self.position_margin is not None else 0.0,
            self.velocity_max if self.velocity_max is not None else -1.0, self.power_cutoff or 0.0, eng._stream()))

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """Restart the windows of the masked lanes (every lane without a mask) with the quantities at the state of their new
        episode; the other lanes keep every tensor, the ring and the counter bit for bit.  Call it after the engine's `start`
        / `reset_lanes`."""
        from . import actuation
        self._launch(actuation.RESTART, self._mask(lane_mask))

    def refresh(self) -> None:
        """One launch on the engine's stream: the quantities at the engine's state, pushed into the window of every lane."""
        from . import actuation
        self._launch(actuation.PUSH, None)


FOOTPOSES_SCALARS = ("reward_foot_positions", "reward_foot_orientations")


def footposes_fieldnames(foot_frame_names):
    """Names of the rows of the tensors of a `FootPoseQuantities` block (`[row][foot]` for the relative ones)."""
    pose = ("X", "Y", "Z", "QuatX", "QuatY", "QuatZ", "QuatW")
    rel = list(foot_frame_names)[:-1]
    return {"mean_pose": [f"FootMean.{e}" for e in pose], "mean_odom_pose": ["FootMeanOdom.X", "FootMeanOdom.Y", "FootMeanOdom.Yaw"],
            "relative_pose": [[f"{n}.Relative{e}" for n in rel] for e in pose],
            "reference_relative_pose": [[f"{n}.ReferenceRelative{e}" for n in rel] for e in pose],
            "tracking_error": [[f"{n}.Error{e}" for n in rel] for e in ("X", "Y", "Z", "AngX", "AngY", "AngZ")],
            "scalars": list(FOOTPOSES_SCALARS)}


class FootPoseQuantities(_PlanBlock):
    """The foot pose quantities of the reference's locomotion layer per lane, from the `pose` of a `FrameKinematics`, F feet in
    the order of `foot_frame_names` (sorted, `sanitize_foot_frame_names`): `mean_pose` `[7][B]` ≙ `MultiFootMeanXYZQuat`
    (quantities/locomotion.py:416-478; quantities/generic.py:950-1062); `mean_odom_pose` `[3][B]` ≙ `MultiFootMeanOdometryPose`
    (:482-557); `relative_pose` `[7][F-1][B]` ≙ `MultiFootRelativeXYZQuat` (:702-810), the pose of every foot but the last in
    the mean pose; `tracking_error` `[6][F-1][B]`: relative position minus reference position and
    `quat_difference(relative quaternion, reference quaternion)`, the errors of `TrackingFootPositionsReward` /
    `TrackingFootOrientationsReward` (compositions/locomotion.py:146-214); `scalars` `[2][B]`, rows `FOOTPOSES_SCALARS`: those two
    rewards with `position_cutoff` / `orientation_cutoff` (None: that row stays zero and its property raises).

    The reference is `reference_relative_pose` `[7][F-1][B]`, a tensor of the block the caller fills (it stands for what
    `QuantityEvalMode.REFERENCE` reads from a trajectory database): zero positions and unit quaternions at first;
    `set_reference_from_current(lane_mask)` copies `relative_pose` into it on the masked lanes.

    Deviation: with three feet or more the mean quaternion is an eigenvector, whose sign LAPACK leaves arbitrary in the
    reference; here it has a non-negative dot product with the quaternion of the first foot.  Yaw, error and rewards do not
    depend on the sign; the relative quaternions flip with it.

    `frames`: the `FrameKinematics` block of the same engine, holding every foot frame; refresh it first.  `refresh()` is one
    launch on the engine's stream, without allocation, copy or synchronisation; `reset(lane_mask)` evaluates the masked lanes
    (every lane without a mask) and keeps the others bit for bit.  The tensors never change identity."""

    def __init__(self, engine, frames: "FrameKinematics", *, foot_frame_names="auto", position_cutoff: Optional[float] = None,
                 orientation_cutoff: Optional[float] = None) -> None:
        from . import _abi, footposes
        if not engine.model.has_freeflyer:
            raise ValueError("Only legged robot with floating base are supported: the model has no free-flyer.")
        if frames._eng is not engine:
            raise ValueError("the frame kinematics block belongs to another engine")
        for cutoff in (position_cutoff, orientation_cutoff):
            if cutoff is not None and not float(cutoff) > 0.0:
                raise ValueError("a reward cutoff must be positive")
        self.plan = footposes.build_plan(engine.model, frames.frame_names, foot_frame_names)
        self._bind(engine)
        self._frames = frames
        self.foot_frame_names = list(self.plan.foot_frame_names)
        self.position_cutoff = None if position_cutoff is None else float(position_cutoff)
        self.orientation_cutoff = None if orientation_cutoff is None else float(orientation_cutoff)
        B, R = engine.batch_size, self.plan.n_feet - 1
        new = lambda *shape: torch.zeros((*shape, B), dtype=engine.dtype, device=engine.device)      # noqa: E731
        self.mean_pose, self.mean_odom_pose, self.scalars = new(7), new(3), new(2)
        self.relative_pose, self.reference_relative_pose, self.tracking_error = new(7, R), new(7, R), new(6, R)
        for t in (self.mean_pose, self.relative_pose, self.reference_relative_pose):
            t[6] = 1.0
        self._io = _abi.FootPosesIO()
        self._create_plan("footposes")

    @property
    def fieldnames(self):
        return footposes_fieldnames(self.foot_frame_names)

    @property
    def reward_foot_positions(self) -> torch.Tensor:
        if self.position_cutoff is None:
            raise ValueError("the block has no position reward: build it with position_cutoff")
        return self.scalars[0]

    @property
    def reward_foot_orientations(self) -> torch.Tensor:
        if self.orientation_cutoff is None:
            raise ValueError("the block has no orientation reward: build it with orientation_cutoff")
        return self.scalars[1]

    def _launch(self, mask: Optional[torch.Tensor]) -> None:
        eng, io, ptr = self._eng, self._io, self._ptr
        io.pose = ptr(self._frames.pose)
        io.lane_mask = ptr(mask, torch.uint8)
        # (one foot: the relative tensors have no column and go in as null pointers)
        for name in ("reference_relative_pose", "mean_pose", "mean_odom_pose", "relative_pose", "tracking_error", "scalars"):
            setattr(io, name, ptr(getattr(self, name)))
        self._check(self._L.jm_block_foot_poses(self._plan, self._dtype, eng.batch_size, self._C.byref(io),
                                                self.position_cutoff or 0.0, self.orientation_cutoff or 0.0, eng._stream()))

    def set_reference_from_current(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """`relative_pose` becomes the reference of the masked lanes (every lane without a mask); the tracking error and the
        rewards follow at the next `refresh` / `reset`."""
        mask = self._mask(lane_mask)
        if mask is None:
            self.reference_relative_pose.copy_(self.relative_pose)
        else:
            torch.where(mask.bool(), self.relative_pose, self.reference_relative_pose, out=self.reference_relative_pose)

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """The quantities at the state of a new episode on the masked lanes (every lane without a mask); the other lanes
        keep every tensor bit for bit.  Call it after the engine's `start` / `reset_lanes` and the reset of `frames`."""
        self._launch(self._mask(lane_mask))

    def refresh(self) -> None:
        """One launch on the engine's stream, behind the refresh of `frames`."""
        self._launch(None)


def support_fieldnames(contact_names):
    """Names of the rows of the tensors of a `SupportPolygon` block (`vertex_index` counts in `contact_names`)."""
    from .support import MAX_POINTS, SCALARS
    return {"n_vertices": ["SupportPolygon.VertexCount"], "vertex_index": [f"SupportPolygon.Vertex{k}" for k in range(MAX_POINTS)],
            "vertices": [[f"SupportPolygon.Vertex{k}.{e}" for k in range(MAX_POINTS)] for e in ("X", "Y")],
            "center": ["SupportPolygon.CenterX", "SupportPolygon.CenterY"], "scalars": list(SCALARS),
            "points": list(contact_names)}


class SupportPolygon(_PlanBlock):
    """The projected support polygon of the reference's toolbox per lane (toolbox/quantities/locomotion.py:22-239,
    toolbox/math/qhull.py, toolbox/compositions/locomotion.py:15-115), from the `pose` of a `FrameKinematics` and the `zmp` /
    `odom_pose` of a `LocomotionQuantities`: `n_vertices` `[B]` and `vertex_index` `[16][B]` (int32; indices into the model's
    contact points in the reference's vertex order, -1 behind the last vertex), `vertices` `[2][16][B]` (NaN behind the last
    vertex) and `center` `[2][B]` ≙ `ProjectedSupportPolygon` (`ConvexHull2D.indices`, `.vertices`, `.center`); `scalars`
    `[2][B]`, rows `support.SCALARS`: `stability_margin` ≙ `StabilityMarginProjectedSupportPolygon` (minus the signed distance
    of the ZMP from the border; -inf where the ZMP is NaN, a robot in free fall) and `reward_robustness` ≙ `MaximizeRobustness`
    with `cutoff_inner` / `cutoff_outer` (both None: the row stays zero and the property raises).

    `frames`: the `FrameKinematics` block of the same engine holding every contact frame; `locomotion`: the
    `LocomotionQuantities` block of the same engine and the same `frames`; refresh both first.  `reference_frame` ('LOCAL' or
    'LOCAL_WORLD_ALIGNED') defaults to the frame of `locomotion.zmp`.  The margin is evaluated in the one frame the block has:
    the polygon and the ZMP must be in the same frame, another `reference_frame` than `locomotion`'s `zmp_reference_frame`
    raises (unless `locomotion.zmp` is None).  The reference evaluates the margin in LOCAL_WORLD_ALIGNED; in LOCAL the margin
    equals that value up to round-off, because the map into the odometry frame is rigid and keeps distances.  Where
    `locomotion.zmp` is None (a reference state without accelerations) the block gives the polygon only and `scalars` is None.
    A pair of `state=` blocks (`QuantityEvalMode.REFERENCE`) works as it is: the block only reads their tensors.

    Deviations.  The reference prunes, on the host, the contact points that are not vertices of the 3D hull of their body, which
    does not change the polygon; here every contact point is a candidate, and a model with more than 16 contact points is
    refused.  A cutoff of zero where the other is given is refused: the reference accepts it and would divide 0 by 0 at a
    margin of exactly 0.  One cutoff without the other is refused as well (the reference takes both).

    `refresh()` is one launch on the engine's stream, without allocation, copy or synchronisation; `reset(lane_mask)` evaluates
    the masked lanes (every lane without a mask) and keeps the others bit for bit.  The tensors never change identity."""

    def __init__(self, engine, frames: "FrameKinematics", locomotion: "LocomotionQuantities", *, reference_frame=None,
                 cutoff_inner: Optional[float] = None, cutoff_outer: Optional[float] = None) -> None:
        from . import _abi, support
        from .locomotion import odometry_frame
        support.check_model(engine.model)
        if frames._eng is not engine:
            raise ValueError("the frame kinematics block belongs to another engine")
        if locomotion._eng is not engine:
            raise ValueError("the locomotion quantities block belongs to another engine")
        if locomotion._frames is not frames:
            raise ValueError("the locomotion quantities block reads another frame kinematics block")
        for cutoff in (cutoff_inner, cutoff_outer):
            if cutoff is not None and not float(cutoff) >= 0.0:
                raise ValueError("The inner and outer cutoff thresholds must both be positive.")
        if (cutoff_inner is None) != (cutoff_outer is None):
            raise ValueError("the robustness reward needs cutoff_inner and cutoff_outer together")
        if cutoff_inner is not None and (float(cutoff_inner) == 0.0 or float(cutoff_outer) == 0.0):
            raise ValueError("a cutoff of zero is refused: the reward would divide 0 by 0 at a margin of 0")
        zmp_frame = int(locomotion.plan.arrays["zmp_frame"])
        frame = zmp_frame if reference_frame is None else odometry_frame(reference_frame)
        self.plan = support.build_plan(engine.model, frames.frame_names, frame)
        if locomotion.zmp is not None and frame != zmp_frame:
            names = ("LOCAL", "LOCAL_WORLD_ALIGNED")
            raise ValueError(f"reference_frame {names[frame]} differs from the zmp_reference_frame {names[zmp_frame]} of the "
                             "locomotion quantities block: the margin is evaluated in one frame")
        self._bind(engine)
        self._frames, self._locomotion = frames, locomotion
        self.reference_frame = frame
        self.contact_names = list(self.plan.contact_names)
        self.cutoff_inner = None if cutoff_inner is None else float(cutoff_inner)
        self.cutoff_outer = None if cutoff_outer is None else float(cutoff_outer)
        B, M = engine.batch_size, support.MAX_POINTS
        new = lambda *shape, dtype=engine.dtype: torch.zeros((*shape, B), dtype=dtype, device=engine.device)      # noqa: E731
        self.n_vertices, self.vertex_index = new(dtype=torch.int32), new(M, dtype=torch.int32)
        self.vertices, self.center = new(2, M), new(2)
        self.scalars = new(2) if locomotion.zmp is not None else None
        self._io = _abi.SupportIO()
        self._create_plan("support")

    @property
    def fieldnames(self):
        return support_fieldnames(self.contact_names)

    @property
    def stability_margin(self) -> torch.Tensor:
        if self.scalars is None:
            raise ValueError("the block has no margin: the locomotion quantities block has no zmp")
        return self.scalars[0]

    @property
    def reward_robustness(self) -> torch.Tensor:
        if self.scalars is None or self.cutoff_inner is None:
            raise ValueError("the block has no reward: build it with cutoff_inner and cutoff_outer (and a zmp)")
        return self.scalars[1]

    def _launch(self, mask: Optional[torch.Tensor]) -> None:
        eng, io, loco, ptr = self._eng, self._io, self._locomotion, self._ptr
        io.pose, io.odom_pose, io.zmp = ptr(self._frames.pose), ptr(loco.odom_pose), ptr(loco.zmp)
        io.lane_mask = ptr(mask, torch.uint8)
        io.n_vertices, io.vertex_index = ptr(self.n_vertices, torch.int32), ptr(self.vertex_index, torch.int32)
        io.vertices, io.center, io.scalars = ptr(self.vertices), ptr(self.center), ptr(self.scalars)
        self._check(self._L.jm_block_support_polygon(self._plan, self._dtype, eng.batch_size, self._C.byref(io),
                                                     self.cutoff_inner or 0.0, self.cutoff_outer or 0.0, eng._stream()))

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """The quantities at the state of a new episode on the masked lanes (every lane without a mask); the other lanes
        keep every tensor bit for bit.  Call it after the reset of `frames` and of `locomotion`."""
        self._launch(self._mask(lane_mask))

    def refresh(self) -> None:
        """One launch on the engine's stream, behind the refresh of `frames` and of `locomotion`."""
        self._launch(None)


def tracking_fieldnames(foot_frame_names, motor_names):
    """Names of the rows of the tensors of a `TrackingWindows` block (`[row][foot]` for the foot reference)."""
    from .tracking import SCALARS
    odom = ("X", "Y", "Yaw")
    return {"reference_odom_pose": [f"ReferenceOdom.{e}" for e in odom], "delta_odom": [f"DeltaOdom.{e}" for e in odom],
            "delta_odom_reference": [f"ReferenceDeltaOdom.{e}" for e in odom],
            "reference_relative_pose": footposes_fieldnames(foot_frame_names)["reference_relative_pose"] if foot_frame_names else [],
            "reference_position": [f"{n}.ReferencePosition" for n in motor_names], "scalars": list(SCALARS)}


class TrackingWindows(_PlanBlock):
    """The trajectory-tracking windows of the reference's composition layer per lane, over sliding windows of environment
    steps: `delta_odom`, `delta_odom_reference` `[3][B]` ≙ `DeltaBaseOdometryPosition` / `DeltaBaseOdometryOrientation`
    (quantities/locomotion.py:1537-1693) of the true and of the reference odometry pose; `scalars` `[6][B]`, rows
    `tracking.SCALARS`: `drift_odom_position`, `drift_odom_orientation` ≙ the values of
    `DriftTrackingBaseOdometryPositionTermination` / `...OrientationTermination` (compositions/locomotion.py:623-736),
    `reward_odom_pose` ≙ `DriftTrackingBaseOdometryPoseReward` (:85-120) with `odometry_cutoff`, `shift_foot_positions`,
    `shift_foot_orientations` ≙ `ShiftTrackingFootOdometryPositionsTermination` / `...OrientationsTermination` (:739-867),
    `shift_motor_positions` ≙ `ShiftTrackingMotorPositionsTermination` (compositions/generic.py:664-716).  A row whose family or
    cutoff is absent stays zero and its property raises.

    A horizon selects its family and names its source block, of the same engine: `odometry_horizon` reads `odom_pose` of
    `locomotion` (`LocomotionQuantities`), `foot_horizon` `relative_pose` and `reference_relative_pose` of `foot_poses`
    (`FootPoseQuantities`, two feet or more: the foot reference stays that block's tensor), `motor_horizon` `position` of
    `actuation` (`ActuatedJointQuantities`, joint side).  Refresh the source blocks first.  The other references are tensors of
    this block the caller fills (they stand for what `QuantityEvalMode.REFERENCE` reads from a trajectory database):
    `reference_odom_pose` `[3][B]` and `reference_position` `[M][B]`, zero at first; `set_reference_from_current(lane_mask)`
    copies the current true values into every reference on the masked lanes.

    The windows are state of the block: `count` `[B]`, the number of pushes of every lane since its restart, and the rings
    `odom_ring`, `yaw_prev`, `yaw_ring`, `foot_ring`, `motor_ring` (layouts: include/jiminy_hip.h).  `reset(lane_mask)` restarts
    the windows of the masked lanes (every lane without a mask) and keeps the other lanes bit for bit, rings and counter
    included; `refresh()` pushes one environment step on every lane: call it once per step.  Both are one launch on the
    engine's stream, without allocation, copy or synchronisation, and no launch argument changes from step to step.  The
    tensors never change identity.  One window per family and block: other horizons take a second block."""

    def __init__(self, engine, *, locomotion: Optional["LocomotionQuantities"] = None, foot_poses: Optional["FootPoseQuantities"] = None,
                 actuation: Optional["ActuatedJointQuantities"] = None, odometry_horizon: Optional[float] = None,
                 foot_horizon: Optional[float] = None, motor_horizon: Optional[float] = None,
                 odometry_cutoff: Optional[float] = None, step_dt: float) -> None:
        from . import _abi, tracking
        for horizon, block, what, keyword in ((odometry_horizon, locomotion, "odometry_horizon", "locomotion"),
                                              (foot_horizon, foot_poses, "foot_horizon", "foot_poses"),
                                              (motor_horizon, actuation, "motor_horizon", "actuation")):
            if horizon is not None and block is None:
                raise ValueError(f"{what} reads the {keyword} block: give {keyword} as well")
            if block is not None and block._eng is not engine:
                raise ValueError(f"the {keyword} block belongs to another engine")
        if odometry_cutoff is not None and not float(odometry_cutoff) > 0.0:
            raise ValueError("a reward cutoff must be positive")
        if odometry_cutoff is not None and odometry_horizon is None:
            raise ValueError("odometry_cutoff rewards the drift of the odometry pose: give odometry_horizon as well")
        if motor_horizon is not None and actuation.motor_side:
            raise ValueError("the motor windows read joint-side positions: the actuation block was built with motor_side=True")
        self.plan = tracking.build_plan(step_dt=step_dt, odometry_horizon=odometry_horizon, foot_horizon=foot_horizon,
                                        motor_horizon=motor_horizon,
                                        n_feet=None if foot_horizon is None else foot_poses.plan.n_feet,
                                        n_motors=None if motor_horizon is None else actuation.plan.n_motors)
        self._bind(engine)
        self._locomotion = locomotion if odometry_horizon is not None else None
        self._foot_poses = foot_poses if foot_horizon is not None else None
        self._actuation = actuation if motor_horizon is not None else None
        self.odometry_horizon = None if odometry_horizon is None else float(odometry_horizon)
        self.foot_horizon = None if foot_horizon is None else float(foot_horizon)
        self.motor_horizon = None if motor_horizon is None else float(motor_horizon)
        self.odometry_cutoff = None if odometry_cutoff is None else float(odometry_cutoff)
        B, p = engine.batch_size, self.plan
        new = lambda *shape, dtype=engine.dtype: torch.zeros((*shape, B), dtype=dtype, device=engine.device)      # noqa: E731
        self.scalars, self.count = new(6), new(dtype=torch.int32)
        self.reference_odom_pose = self.delta_odom = self.delta_odom_reference = None
        self.odom_ring = self.yaw_prev = self.yaw_ring = self.foot_ring = self.reference_position = self.motor_ring = None
        if p.max_stack_odom:
            self.reference_odom_pose, self.delta_odom, self.delta_odom_reference = new(3), new(3), new(3)
            self.odom_ring, self.yaw_prev, self.yaw_ring = new(p.max_stack_odom, 4), new(2), new(p.max_stack_odom - 1, 2)
        if p.max_stack_foot:
            self.foot_ring = new(2, p.max_stack_foot)
        if p.max_stack_motor:
            self.reference_position, self.motor_ring = new(p.n_motors), new(p.max_stack_motor)
        self._io = _abi.TrackingIO()
        self._create_plan("tracking")

    @property
    def fieldnames(self):
        feet = self._foot_poses.foot_frame_names if self._foot_poses is not None else []
        motors = self._actuation.plan.motor_names if self._actuation is not None else []
        return tracking_fieldnames(feet, motors)

    @property
    def reference_relative_pose(self) -> torch.Tensor:
        """The reference of the foot windows: the tensor of the foot pose quantities block."""
        if self._foot_poses is None:
            raise ValueError("the block has no foot windows: build it with foot_horizon")
        return self._foot_poses.reference_relative_pose

    def _scalar(self, row: int, present: bool, keyword: str) -> torch.Tensor:
        if not present:
            raise ValueError(f"the block does not evaluate this value: build it with {keyword}")
        return self.scalars[row]

    @property
    def drift_odom_position(self) -> torch.Tensor:
        return self._scalar(0, self._locomotion is not None, "odometry_horizon")

    @property
    def drift_odom_orientation(self) -> torch.Tensor:
        return self._scalar(1, self._locomotion is not None, "odometry_horizon")

    @property
    def reward_odom_pose(self) -> torch.Tensor:
        return self._scalar(2, self.odometry_cutoff is not None, "odometry_cutoff")

    @property
    def shift_foot_positions(self) -> torch.Tensor:
        return self._scalar(3, self._foot_poses is not None, "foot_horizon")

    @property
    def shift_foot_orientations(self) -> torch.Tensor:
        return self._scalar(4, self._foot_poses is not None, "foot_horizon")

    @property
    def shift_motor_positions(self) -> torch.Tensor:
        return self._scalar(5, self._actuation is not None, "motor_horizon")

    def _launch(self, mode: int, mask: Optional[torch.Tensor]) -> None:
        eng, io, ptr = self._eng, self._io, self._ptr
        io.odom_pose = ptr(self._locomotion.odom_pose) if self._locomotion is not None else None
        io.relative_pose = ptr(self._foot_poses.relative_pose) if self._foot_poses is not None else None
        io.reference_relative_pose = ptr(self._foot_poses.reference_relative_pose) if self._foot_poses is not None else None
        io.position = ptr(self._actuation.position) if self._actuation is not None else None
        io.lane_mask = ptr(mask, torch.uint8)
        io.count = ptr(self.count, torch.int32)
        for name in ("reference_odom_pose", "reference_position", "odom_ring", "yaw_prev", "yaw_ring", "foot_ring", "motor_ring",
                     "delta_odom", "delta_odom_reference", "scalars"):
            setattr(io, name, ptr(getattr(self, name)))
        self._check(self._L.jm_block_tracking(self._plan, self._dtype, eng.batch_size, self._C.byref(io), mode,
                                              self.odometry_cutoff or 0.0, eng._stream()))

    def set_reference_from_current(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """The current true values become the references of the masked lanes (every lane without a mask): the odometry pose,
        the motor positions and, through `FootPoseQuantities.set_reference_from_current`, the relative foot poses.  The windows
        follow at the next `refresh` / `reset`."""
        mask = self._mask(lane_mask)
        pairs = []
        if self._locomotion is not None:
            pairs.append((self._locomotion.odom_pose, self.reference_odom_pose))
        if self._actuation is not None:
            pairs.append((self._actuation.position, self.reference_position))
        for src, dst in pairs:
            if mask is None:
                dst.copy_(src)
            else:
                torch.where(mask.bool(), src, dst, out=dst)
        if self._foot_poses is not None:
            self._foot_poses.set_reference_from_current(lane_mask)

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """Restart the windows of the masked lanes (every lane without a mask) at the values of their new episode; the other
        lanes keep every tensor, the rings and the counter bit for bit.  Call it after the reset of the source blocks."""
        from . import tracking
        self._launch(tracking.RESTART, self._mask(lane_mask))

    def refresh(self) -> None:
        """One launch on the engine's stream, behind the refresh of the source blocks: one environment step pushed into the
        windows of every lane."""
        from . import tracking
        self._launch(tracking.PUSH, None)


def trajectory_fieldnames(model, fields: int, motor_names):
    """Names of the rows of the tensors of a `ReferenceTrajectory` block."""
    from .trajectory import HAS_A, HAS_COMMAND, HAS_V, STATUS
    names = {"q": [f"ReferenceQ.{i}" for i in range(model.nq)], "odom_pose": [f"ReferenceOdom.{e}" for e in ("X", "Y", "Yaw")],
             "position": [f"{n}.ReferencePosition" for n in motor_names], "status": list(STATUS)}
    if fields & HAS_V:
        names["v"] = [f"ReferenceV.{i}" for i in range(model.nv)]
    if fields & HAS_A:
        names["a"] = [f"ReferenceA.{i}" for i in range(model.nv)]
    if fields & HAS_COMMAND:
        names["command"] = [f"{m.name}.ReferenceCommand" for m in model.motors]
    return names


class ReferenceTrajectory(_PlanBlock):
    """The state of a recorded trajectory at every lane's own time: what `QuantityEvalMode.REFERENCE` reads.  ≙
    `DatasetTrajectoryQuantity` (bases/quantities.py:870-1210) over `Trajectory.get` (jiminy_py/dynamics.py:296-388).

    `dataset` is `{name: (jiminy_amd.trajectory.Trajectory, mode)}`, ordered like the reference's registry, mode "raise",
    "wrap" or "clip"; it is copied to the device once and immutable afterwards (the reference's `lock()`).  `names` lists the
    trajectories in order.  Per lane: `trajectory` `[B]` (int32, the selected trajectory) and `time_offset` `[B]` (float64),
    written by `select(name_or_indices, lane_mask=None, time_offset_ratio=0.0)`: `time_offset = t_start + ratio * (t_end -
    t_start)` of the selected trajectory (:1171-1174), the ratio a number or a `[B]` tensor.

    `query(time, lane_mask=None)` evaluates the selected trajectories at `time + time_offset` (`time`: float64 `[B]`, the
    lanes' episode times) into `q` `[nq][B]`, `v`, `a` `[nv][B]`, `command` `[n_motors][B]` (the fields the dataset carries;
    None otherwise), `odom_pose` `[3][B]` (x, y, yaw of the free-flyer, the function of `LocomotionQuantities.odom_pose`; None
    without a free-flyer), `position` `[M][B]` (`q` at the motors' rows, joint side) and `status` `[3][B]` (int32: flags,
    `n_steps` of a wrapping time, index of the right sample).  `out_of_range` is bit 0 of the flags: the lanes where the
    reference raises "Query time out-of-range." (mode "raise"); they carry the state at the clipped time.  One launch on the
    engine's stream, without allocation, copy or synchronisation; no launch argument changes from call to call and the
    tensors never change identity.  Lanes outside `lane_mask` keep every tensor bit for bit.

    `bind_references(tracking)` makes the block write `odom_pose` / `position` straight into `reference_odom_pose` /
    `reference_position` of a `TrackingWindows` block (these then ARE this block's tensors).  `actuation` (an
    `ActuatedJointQuantities` block) names the motors of `position`; default: the model's."""

    def __init__(self, engine, dataset, *, actuation: Optional["ActuatedJointQuantities"] = None) -> None:
        import os

        import numpy as np

        from . import _abi, trajectory
        if os.environ.get("JIMINY_AMD_TENSOR_BLOCKS", "0") == "1":
            raise NotImplementedError("the reference trajectories have no tensor-program form (JIMINY_AMD_TENSOR_BLOCKS=1): "
                                      "the lookup exists as the HIP kernel only")
        if actuation is not None and actuation._eng is not engine:
            raise ValueError("the actuation block belongs to another engine")
        motor_rows = None if actuation is None else [int(i) for i in actuation.plan.arrays["idx_q"]]
        self.plan = trajectory.build_plan(engine.model, dataset, motor_rows)
        self.names = list(self.plan.names)
        self._motor_names = list(actuation.plan.motor_names) if actuation is not None else \
            [m.name for m in engine.model.motors][:self.plan.n_motors]
        self._bind(engine)
        B, p = engine.batch_size, self.plan
        new = lambda *shape, dtype=engine.dtype: torch.zeros((*shape, B), dtype=dtype, device=engine.device)      # noqa: E731
        self.q = new(p.nq)
        self.v = new(p.nv) if p.fields & trajectory.HAS_V else None
        self.a = new(p.nv) if p.fields & trajectory.HAS_A else None
        self.command = new(p.n_command) if p.fields & trajectory.HAS_COMMAND else None
        self.odom_pose = new(3) if p.has_freeflyer else None
        self.position = new(p.n_motors) if p.n_motors else None
        self.status = new(3, dtype=torch.int32)
        self.trajectory = new(dtype=torch.int32)
        self.time_offset = new(dtype=torch.float64)
        self._interval = torch.as_tensor(p.time_interval, dtype=torch.float64, device=engine.device)
        self.time_offset.fill_(float(p.time_interval[0, 0]))
        self._io = _abi.TrajectoryIO()
        self.plan.dtype = np.float64 if engine.dtype == torch.float64 else np.float32
        self._create_plan("trajectory")

    @property
    def fieldnames(self):
        return trajectory_fieldnames(self._eng.model, self.plan.fields, self._motor_names)

    @property
    def out_of_range(self) -> torch.Tensor:
        """`[B]` bool: the query time of the lane was out of range in mode "raise" at the last `query`."""
        return (self.status[0] & 1).bool()

    def select(self, name_or_indices, lane_mask: Optional[torch.Tensor] = None, time_offset_ratio=0.0) -> None:
        """Select a trajectory by name (every masked lane the same) or by a `[B]` tensor of indices, and set the time offset
        of the masked lanes (every lane without a mask) from `time_offset_ratio`, a number or a `[B]` tensor."""
        eng, B = self._eng, self._eng.batch_size
        if isinstance(name_or_indices, str):
            if name_or_indices not in self.names:
                raise KeyError(f"no trajectory named '{name_or_indices}' (registered: {', '.join(self.names)})")
            index = torch.full((B,), self.names.index(name_or_indices), dtype=torch.int64, device=eng.device)
        else:
            index = torch.as_tensor(name_or_indices, device=eng.device).to(torch.int64)
            if index.ndim == 0:
                index = index.expand(B)
            if tuple(index.shape) != (B,):
                raise ValueError(f"the trajectory indices must have shape ({B},)")
        mask = None if lane_mask is None else self._mask(lane_mask).bool()
        chosen = index if mask is None else index[mask]
        if chosen.numel() and (int(chosen.min()) < 0 or int(chosen.max()) >= len(self.names)):
            raise IndexError(f"trajectory index out of range [0, {len(self.names)})")
        ratio = torch.as_tensor(time_offset_ratio, dtype=torch.float64, device=eng.device)
        if ratio.ndim == 0:
            ratio = ratio.expand(B)
        if tuple(ratio.shape) != (B,):
            raise ValueError(f"time_offset_ratio must be a number or have shape ({B},)")
        interval = self._interval[index.clamp(0, len(self.names) - 1)]
        offset = interval[:, 0] + ratio * (interval[:, 1] - interval[:, 0])
        if mask is None:
            self.trajectory.copy_(index)
            self.time_offset.copy_(offset)
        else:
            torch.where(mask, index.to(torch.int32), self.trajectory, out=self.trajectory)
            torch.where(mask, offset, self.time_offset, out=self.time_offset)

    def bind_references(self, tracking: "TrackingWindows") -> None:
        """Write `odom_pose` / `position` straight into the references of a `TrackingWindows` block of the same engine."""
        if tracking._eng is not self._eng:
            raise ValueError("the tracking block belongs to another engine")
        if tracking.reference_odom_pose is not None:
            if self.odom_pose is None:
                raise ValueError("the odometry windows need the reference of a free-flyer: the model has none")
            self.odom_pose = tracking.reference_odom_pose
        if tracking.reference_position is not None:
            if self.position is None or tuple(self.position.shape) != tuple(tracking.reference_position.shape):
                raise ValueError("the motor windows and the trajectory block do not describe the same motors")
            self.position = tracking.reference_position

    def query(self, time: torch.Tensor, lane_mask: Optional[torch.Tensor] = None) -> None:
        """One launch on the engine's stream: the state of every (masked) lane's trajectory at `time + time_offset`."""
        eng, io = self._eng, self._io
        if time.dtype != torch.float64 or tuple(time.shape) != (eng.batch_size,) or time.device != eng.device or \
                not time.is_contiguous():
            raise ValueError(f"time must be a contiguous float64 tensor of shape ({eng.batch_size},) on the engine's device")
        mask = self._mask(lane_mask)
        io.time, io.trajectory, io.time_offset = time.data_ptr(), self.trajectory.data_ptr(), self.time_offset.data_ptr()
        io.lane_mask = self._ptr(mask, torch.uint8)
        for name in ("q", "v", "a", "command", "odom_pose", "position"):
            setattr(io, name, self._ptr(getattr(self, name)))
        io.status = self.status.data_ptr()
        self._check(self._L.jm_block_trajectory_state(self._plan, self._dtype, eng.batch_size, self._C.byref(io), eng._stream()))


def integrate_zoh(state: torch.Tensor, state_min: torch.Tensor, state_max: torch.Tensor,
                  dt: float) -> None:
    """≙ `integrate_zoh` (proportional_derivative_controller.py:23-98), in place.

    `state` is `[3][M][B]` (position, velocity, acceleration); bounds are `[3][M]` or `[3][M][B]`.
    """
    assert dt >= 0.0, "Integration backward in time is not supported."
    if abs(dt) < 1e-9:
        return
    if state_min.dim() == 2:
        state_min, state_max = state_min[..., None], state_max[..., None]
    position, velocity, acceleration = state[0], state[1], state[2]
    p_min, v_min, a_min = state_min[0], state_min[1], state_min[2]
    p_max, v_max, a_max = state_max[0], state_max[1], state_max[2]
    acc = torch.minimum(torch.maximum(acceleration, a_min), a_max)
    v_prev = velocity.clone()
    vel = velocity + acc * dt
    vel = torch.minimum(torch.maximum(vel, v_min), v_max)
    # slow down early enough not to violate the acceleration limit when hitting position bounds
    horizon = torch.clamp_min(torch.trunc(v_prev.abs() / a_max / dt) * dt, dt)
    d_min = p_min - position
    d_max = p_max - position
    drift = 0.5 * (horizon * (horizon - dt)) * a_max
    far = horizon > dt
    d_min = torch.where(far, d_min - drift, d_min)
    d_max = torch.where(far, d_max + drift, d_max)
    vel = torch.minimum(torch.maximum(vel, d_min / horizon), d_max / horizon)
    # velocity after hitting bounds must be cancellable in a single step
    fast = vel.abs() > dt * a_max
    safe = torch.where(fast, vel, torch.ones_like(vel))
    lo = -torch.clamp_min(d_min / safe, dt) * a_max
    hi = torch.clamp_min(d_max / safe, dt) * a_max
    vel = torch.where(fast, torch.minimum(torch.maximum(vel, lo), hi), vel)
    state[2].copy_((vel - v_prev) / dt)
    state[1].copy_(vel)
    state[0].copy_(position + dt * vel)


TRACKING_REWARD_TERMS = ("base_height", "odometry_velocity", "capture_point", "joint_positions")


def tracking_rewards_fieldnames(motor_names):
    """Names of the rows of the tensors of a `TrackingRewards` block (`value` and `reference` share theirs)."""
    rows = ["BaseHeight", "OdometryVelocity.X", "OdometryVelocity.Y", "OdometryVelocity.Yaw", "CapturePoint.X", "CapturePoint.Y"]
    rows += [f"{n}.Position" for n in motor_names]
    return {"value": rows, "reference": list(rows), "rewards": [f"reward_{t}" for t in TRACKING_REWARD_TERMS]}


class TrackingRewards(_PlanBlock):
    """The tracking rewards of the reference's composition layer on balance quantities per lane: a quantity in
    `QuantityEvalMode.TRUE` against the same quantity in `QuantityEvalMode.REFERENCE` ≙ `TrackingQuantityReward`
    (compositions/generic.py:64-122).  Terms (`TRACKING_REWARD_TERMS`, the rows of `rewards` `[4][B]`): the base height ≙
    `TrackingBaseHeightReward` (compositions/locomotion.py:33-51), root z minus the lowest contact frame z of the `pose` of
    `frames` / `reference_frames`; the odometry velocity ≙ `TrackingBaseOdometryVelocityReward` (:54-72), rows (0, 1, 5) of the
    step-average velocity of 'root_joint' turned by its `quat_no_yaw` (both blocks with `average=True`, the column LOCAL); the
    capture point ≙ `TrackingCapturePointReward` (:123-143), the `dcm` of `locomotion` / `reference_locomotion`, both built
    with `dcm_reference_frame="LOCAL"`; the joint positions ≙ `TrackingActuatedJointPositionsReward`
    (compositions/generic.py:125-150), `actuation.position` against `trajectory.position`.  `value` and `reference`
    `[6 + n_motors][B]` hold the two sides concatenated (height 1, velocity 3, capture point 2, positions), `rewards` is
    `radial_basis_function(value - reference, cutoff, 2)`.  A term whose cutoff is None is skipped: its rows stay zero.

    `refresh()` is one launch on the engine's stream behind the refresh of every block it reads, `reset(lane_mask)` the same
    on the masked lanes (every lane without a mask), the others keeping every bit.  No allocation, copy or synchronisation;
    the tensors never change identity."""

    def __init__(self, engine, *, frames=None, reference_frames=None, locomotion=None, reference_locomotion=None, actuation=None,
                 trajectory=None, base_height_cutoff: Optional[float] = None, odometry_velocity_cutoff: Optional[float] = None,
                 capture_point_cutoff: Optional[float] = None, joint_positions_cutoff: Optional[float] = None) -> None:
        import os

        from . import _abi, trackrewards
        from . import frames as frames_
        if os.environ.get("JIMINY_AMD_TENSOR_BLOCKS", "0") == "1":
            raise NotImplementedError("the tracking rewards have no tensor-program form (JIMINY_AMD_TENSOR_BLOCKS=1): "
                                      "they exist as the HIP kernel only")
        cutoffs = (base_height_cutoff, odometry_velocity_cutoff, capture_point_cutoff, joint_positions_cutoff)
        for cutoff in cutoffs:
            if cutoff is not None and not float(cutoff) > 0.0:
                raise ValueError("a reward cutoff must be positive")
        for blk in (frames, reference_frames, locomotion, reference_locomotion, actuation, trajectory):
            if blk is not None and blk._eng is not engine:
                raise ValueError("a block the tracking rewards read belongs to another engine")
        if (base_height_cutoff is not None or odometry_velocity_cutoff is not None) and (frames is None or reference_frames is None):
            raise ValueError("the base height and the odometry velocity read the frame kinematics blocks of both sides: "
                             "pass frames and reference_frames")
        if odometry_velocity_cutoff is not None:
            for blk in (frames, reference_frames):
                if not blk.average:
                    raise ValueError("the odometry velocity reads the step average of the root frame: build both frame "
                                     "kinematics blocks with average=True")
                if blk.plan.modes[blk.index("root_joint")] != frames_.LOCAL:
                    raise ValueError("the odometry velocity reads the LOCAL step-average velocity of 'root_joint': a frame "
                                     "kinematics block holds it in another reference frame")
        if capture_point_cutoff is not None:
            if locomotion is None or reference_locomotion is None:
                raise ValueError("the capture point reads the locomotion blocks of both sides: pass locomotion and "
                                 "reference_locomotion")
            for blk in (locomotion, reference_locomotion):
                if blk.plan.arrays["dcm_frame"] != frames_.LOCAL:
                    raise ValueError("the capture point is tracked in the odometry frame: build both locomotion blocks with "
                                     "dcm_reference_frame='LOCAL'")
        if joint_positions_cutoff is not None and (actuation is None or trajectory is None or trajectory.position is None):
            raise ValueError("the joint positions read actuation.position and trajectory.position: pass actuation and a "
                             "trajectory built with it")
        n_motors = 0 if actuation is None else int(actuation.position.shape[0])
        self.plan = trackrewards.build_plan(engine.model, None if frames is None else frames.frame_names,
                                            None if reference_frames is None else reference_frames.frame_names, n_motors)
        self._bind(engine)
        self._blocks = (frames, reference_frames, locomotion, reference_locomotion, actuation, trajectory)
        self.cutoffs = tuple(None if c is None else float(c) for c in cutoffs)
        self._cutoff = (self._C.c_double * 4)(*[c or 0.0 for c in self.cutoffs])
        B = engine.batch_size
        new = lambda rows: torch.zeros((rows, B), dtype=engine.dtype, device=engine.device)      # noqa: E731
        self.value, self.reference, self.rewards = new(self.plan.rows), new(self.plan.rows), new(4)
        self._io = _abi.TrackRewardsIO()
        self._create_plan("trackrewards")

    @property
    def fieldnames(self):
        return tracking_rewards_fieldnames([m.name for m in self._eng.model.motors][:self.plan.n_motors])

    def reward(self, term: str) -> torch.Tensor:
        """The row of `rewards` of a term of `TRACKING_REWARD_TERMS`."""
        return self.rewards[TRACKING_REWARD_TERMS.index(term)]

    def _launch(self, mask: Optional[torch.Tensor]) -> None:
        eng, io, ptr = self._eng, self._io, self._ptr
        frames, reference_frames, locomotion, reference_locomotion, actuation, trajectory = self._blocks
        get = lambda blk, name: None if blk is None else ptr(getattr(blk, name))      # noqa: E731
        io.pose, io.pose_reference = get(frames, "pose"), get(reference_frames, "pose")
        io.v_avg, io.quat_no_yaw = get(frames, "average_velocity"), get(frames, "quat_no_yaw")
        io.v_avg_reference, io.quat_no_yaw_reference = get(reference_frames, "average_velocity"), get(reference_frames, "quat_no_yaw")
        io.dcm, io.dcm_reference = get(locomotion, "dcm"), get(reference_locomotion, "dcm")
        io.position, io.position_reference = get(actuation, "position"), get(trajectory, "position")
        io.lane_mask = ptr(mask, torch.uint8)
        io.value, io.reference, io.rewards = ptr(self.value), ptr(self.reference), ptr(self.rewards)
        self._check(self._L.jm_block_tracking_rewards(self._plan, self._dtype, eng.batch_size, self._C.byref(io), self._cutoff,
                                                      eng._stream()))

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        """The rewards at the state of a new episode on the masked lanes (every lane without a mask); the other lanes keep
        every tensor bit for bit.  Call it after the reset of every block it reads."""
        self._launch(self._mask(lane_mask))

    def refresh(self) -> None:
        """One launch on the engine's stream, behind the refresh of every block it reads."""
        self._launch(None)


class Composition(_PlanBlock):
    """The composition layer of the reference's environments per lane ≙ `ComposedJiminyEnv(reward=..., terminations=[...])`
    (bases/pipeline.py:751-829 over bases/compositions.py, compositions/mixin.py, compositions/generic.py): `reward` is a
    description of `jiminy_amd.compositions` (`RewardTerm`, `SurviveReward`, `AdditiveMixtureReward`,
    `MultiplicativeMixtureReward`) or None, `terminations` a sequence of `compositions.Termination`, in evaluation order;
    their rows are views of tensors other blocks of `engine` own, which must keep their identity.

    `refresh(time, base_terminated, base_truncated, training=True, lane_mask=None)`: `time` `[B]` (engine dtype) is the
    episode time of every lane, the two flags (bool or uint8 `[B]`) are those of the environment below.  Outputs: `terminated`,
    `truncated` (uint8 `[B]`; a lane with a base flag keeps both and evaluates no condition), `trigger` (int32 `[B]`: the
    first condition that fired, -1 for none or a base flag), `reward` `[B]`, `node_value` `[n_nodes][B]` (NaN where a node was
    not evaluated; `info()` gives its rows by name, `node_names` their order) and `violations` (int32 `[B]`: the bit of the
    first node advertised as normalised that left [0, 1], where the reference raises ValueError).  See
    `jiminy_amd.compositions` for the three behaviours of the reference that hold here.

    One launch on the engine's stream, without allocation, copy or synchronisation; lanes outside `lane_mask` keep every
    tensor bit for bit.  The tensors never change identity."""

    def __init__(self, engine, reward=None, terminations=()) -> None:
        import os

        from . import _abi, compositions
        if os.environ.get("JIMINY_AMD_TENSOR_BLOCKS", "0") == "1":
            raise NotImplementedError("the composition layer has no tensor-program form (JIMINY_AMD_TENSOR_BLOCKS=1): "
                                      "it exists as the HIP kernel only")
        self.plan = compositions.build_plan(reward, terminations, engine.batch_size, engine.dtype)
        for t in self.plan.sources:
            if t.device != engine.device:
                raise ValueError("pipeline block tensors must be on the engine's device")
        self._bind(engine)
        self.node_names, self.condition_names = list(self.plan.node_names), list(self.plan.condition_names)
        B = engine.batch_size
        new = lambda *shape, dtype=engine.dtype: torch.zeros((*shape, B), dtype=dtype, device=engine.device)      # noqa: E731
        self.reward, self.node_value = new(), new(self.plan.n_nodes)
        self.terminated, self.truncated = new(dtype=torch.uint8), new(dtype=torch.uint8)
        self.trigger, self.violations = new(dtype=torch.int32), new(dtype=torch.int32)
        self.trigger.fill_(-1)
        self._io = _abi.ComposeIO()
        for s, ptr in enumerate(self.plan.source_ptr):
            self._io.source[s] = ptr
        self._create_plan("compose")

    def info(self) -> Dict[str, torch.Tensor]:
        """≙ the reward's entries of the reference's `info`: the row of `node_value` of every node by name (NaN on the lanes
        where the node was not evaluated)."""
        return {name: self.node_value[n] for n, name in enumerate(self.node_names)}

    def refresh(self, time: torch.Tensor, base_terminated: Optional[torch.Tensor] = None, base_truncated: Optional[torch.Tensor] = None,
                training: bool = True, lane_mask: Optional[torch.Tensor] = None) -> None:
        eng, io, B = self._eng, self._io, self._eng.batch_size
        time_ptr = self._ptr(time)
        if time is not None and tuple(time.shape) != (B,):
            raise ValueError(f"time must have shape ({B},)")
        # (the views of bool flags are held until the launch is issued)
        held = [self._flags(base_terminated, "base_terminated"), self._flags(base_truncated, "base_truncated"),
                self._flags(lane_mask, "lane_mask")]
        io.time = time_ptr
        io.base_terminated, io.base_truncated, io.lane_mask = (None if t is None else t.data_ptr() for t in held)
        io.reward, io.node_value = self.reward.data_ptr(), self.node_value.data_ptr() if self.plan.n_nodes else None
        io.terminated, io.truncated = self.terminated.data_ptr(), self.truncated.data_ptr()
        io.trigger, io.violations = self.trigger.data_ptr(), self.violations.data_ptr()
        self._check(self._L.jm_block_compose(self._plan, self._dtype, B, self._C.byref(io), int(bool(training)), eng._stream()))


class ObservationAssembler(_PlanBlock):
    """The observation the learner reads, assembled per lane ≙ `FlattenObservation(StackObservation(NormalizeObservation(
    ScaleObservation(AdaptLayoutObservation(env)))))` (wrappers/observation_layout.py:36-540, scale.py:31-244, normalize.py:49-114,
    observation_stack.py:40-265, flatten.py) as one launch of `jm_block_observe` (csrc/jm_observe.h).  `obs` is the nested
    observation of the environment, whose leaves are batch-first views of `[rows][B]` tensors other blocks of `engine` own; the
    other arguments are those of the wrappers (`jiminy_amd.observe.build_plan`).

    `out` `(B, W)` in `dtype` and `hist` `[num_stack][D][B]` in the engine dtype are the block's own and never change identity.
    `refresh(shift=True, reset_mask=None, obs=None)`: one launch on the engine's stream, without allocation, copy or
    synchronisation; `shift=False` overwrites the current frame only (`skip_frames_ratio`), `reset_mask` (bool or uint8 `[B]`)
    restarts the older frames of those lanes from zero, `obs` is a new observation of the same environment whose leaves are
    read instead (the data pointers are read at every launch either way).  `reset(lane_mask=None)` zeroes the history."""

    def __init__(self, engine, obs, **spec) -> None:
        import os

        from . import _abi, observe
        if os.environ.get("JIMINY_AMD_TENSOR_BLOCKS", "0") == "1":
            raise NotImplementedError("the observation assembly has no tensor-program form of its own (JIMINY_AMD_TENSOR_BLOCKS=1): "
                                      "wrappers.AssembleObservation runs the chain of tensor wrappers instead")
        self.plan = observe.build_plan(obs, engine_dtype=engine.dtype, **spec)
        self._leaves = observe.source_tensors(obs, self.plan)
        for t in self._leaves:
            if t.device != engine.device:
                raise ValueError("pipeline block tensors must be on the engine's device")
        self._bind(engine)
        self._observe = observe
        # (input and output dtype of the launch: `_dtype`, the engine's, is not what this block passes)
        code = lambda dt: _abi.JM_F64 if dt == torch.float64 else _abi.JM_F32      # noqa: E731
        self._dtype_in, self._dtype_out = code(self.plan.dtype_in), code(self.plan.dtype_out)
        B = engine.batch_size
        self.hist = torch.zeros((self.plan.num_stack, self.plan.n_elements, B), dtype=engine.dtype, device=engine.device)
        self.out = torch.zeros((B, self.plan.n_positions), dtype=self.plan.dtype_out, device=engine.device)
        observe.check_no_alias(self.out, [(f"observation leaf {p}", t) for p, t in zip(self.plan.source_paths, self._leaves)])
        self._io = _abi.ObserveIO()
        self._io.hist, self._io.out = self.hist.data_ptr(), self.out.data_ptr()
        self._create_plan("observe")

    def reset(self, lane_mask: Optional[torch.Tensor] = None) -> None:
        if lane_mask is None:
            self.hist.zero_()
        else:
            self.hist.masked_fill_(lane_mask.to(torch.bool), 0)

    def refresh(self, shift: bool = True, reset_mask: Optional[torch.Tensor] = None, obs=None) -> None:
        eng, io, B = self._eng, self._io, self._eng.batch_size
        leaves = self._leaves if obs is None else self._observe.source_tensors(obs, self.plan)
        for s, (t, first) in enumerate(zip(leaves, self._leaves)):
            if t is not first and (t.shape != first.shape or t.stride() != first.stride() or t.dtype != first.dtype or t.device != first.device):
                raise ValueError(f"observation leaf {self.plan.source_paths[s]} changed its shape, strides, dtype or device")
            io.source[s] = t.data_ptr()
        reset_mask = self._flags(reset_mask, "reset_mask")
        io.reset_mask = None if reset_mask is None else reset_mask.data_ptr()
        self._check(self._L.jm_block_observe(self._plan, self._dtype_in, self._dtype_out, B, self._C.byref(io), int(bool(shift)),
                                             eng._stream()))


def pd_controller(encoder_data: torch.Tensor, command_state: torch.Tensor,
                  command_state_lower: torch.Tensor, command_state_upper: torch.Tensor,
                  kp: torch.Tensor, kd: torch.Tensor, motors_effort_limit: torch.Tensor,
                  control_dt: float, out: torch.Tensor) -> None:
    """≙ `pd_controller` (proportional_derivative_controller.py:101-163).

    `encoder_data` `[2][M][B]` (position, velocity), `command_state` `[3][M][B]` (updated in
    place), gains / limits `[M]` or `[M][B]`, `out` `[M][B]` = clipped motor torques.
    """
    integrate_zoh(command_state, command_state_lower, command_state_upper, control_dt)
    if kp.dim() == 1:
        kp, kd, motors_effort_limit = kp[:, None], kd[:, None], motors_effort_limit[:, None]
    q_error = command_state[0] - encoder_data[0]
    v_error = command_state[1] - encoder_data[1]
    u = kp * (q_error + kd * v_error)
    out.copy_(torch.minimum(torch.maximum(u, -motors_effort_limit), motors_effort_limit))


def pd_adapter(action: torch.Tensor, order: int, command_state: torch.Tensor,
               command_state_lower: torch.Tensor, command_state_upper: torch.Tensor,
               is_instantaneous: bool, motors_velocity_deadband: Optional[torch.Tensor],
               step_dt: float, out: torch.Tensor) -> None:
    """≙ `pd_adapter` (proportional_derivative_controller.py:166-260): target accelerations
    `[M][B]` to hold over `step_dt` so that the `order`-th derivative of the target reaches `action`."""
    if abs(step_dt) < 1e-9:
        return
    lo, hi = command_state_lower, command_state_upper
    if lo.dim() == 2:
        lo, hi = lo[..., None], hi[..., None]
    db = motors_velocity_deadband
    if db is not None and db.dim() == 1:
        db = db[:, None]
    if is_instantaneous:
        if order == 0:
            velocity = (action - command_state[0]) / step_dt
            velocity = torch.minimum(torch.maximum(velocity, lo[1]), hi[1])
            if db is not None:
                velocity = torch.where(velocity.abs() < db, torch.zeros_like(velocity), velocity)
            command_state[0].add_(velocity * step_dt)
            command_state[1].zero_()
        else:
            if db is not None:
                action = action * (action.abs() > db)
            acceleration = (action - command_state[1]) / step_dt
            acceleration = torch.minimum(torch.maximum(acceleration, lo[2]), hi[2])
            command_state[1].add_(acceleration * step_dt)
        out.zero_()
    else:
        velocity = (action - command_state[0]) / step_dt if order == 0 else action
        velocity = torch.minimum(torch.maximum(velocity, lo[1]), hi[1])
        if db is not None:
            velocity = torch.where(velocity.abs() < db, torch.zeros_like(velocity), velocity)
        out.copy_((velocity - command_state[1]) / step_dt)


def compute_tilt_from_quat(q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """R(q)^T e_z for quaternions `[4][...]` xyzw (reference utils/math.py:1046-1060)."""
    q_x, q_y, q_z, q_w = q[0], q[1], q[2], q[3]
    return (2 * (q_x * q_z - q_y * q_w), 2 * (q_y * q_z + q_w * q_x),
            1 - 2 * (q_x * q_x + q_y * q_y))


def mahony_filter(q: torch.Tensor, omega: torch.Tensor, cf: torch.Tensor, gyro: torch.Tensor,
                  acc: torch.Tensor, bias_hat: torch.Tensor, kp: float, ki: float, dt: float
                  ) -> None:
    """≙ `mahony_filter` (mahony_filter.py:28-101), in place; `q` `[4][K]`, the others `[3][K]`
    with K independent filters (`[...][B]`, or `[...][n_imu][B]` for several IMUs per environment).

    The reference returns early when *no* IMU moves (`(|cf| < 1e-6).all()`); per-lane here: a lane
    whose `cf` is below that threshold keeps its orientation and bias (same values, since its
    update would be the identity up to 1e-6 * dt)."""
    v_x, v_y, v_z = compute_tilt_from_quat(q)
    omega.copy_(gyro - bias_hat)
    a_hat = acc / EARTH_SURFACE_GRAVITY
    omega_mes = torch.stack((a_hat[1] * v_z - a_hat[2] * v_y,
                             a_hat[2] * v_x - a_hat[0] * v_z,
                             a_hat[0] * v_y - a_hat[1] * v_x), 0)
    cf.copy_(omega + kp * omega_mes)
    still = cf.abs() < 1e-6
    if cf.dim() == 3:   # [3][n_imu][B]: the early return of the reference is per environment
        moving = (~still.all(dim=0).all(dim=0))[None, :].expand(cf.shape[1], -1)
    else:
        moving = ~still.all(dim=0)
    theta = torch.sqrt((cf * cf).sum(0))
    safe_theta = torch.where(moving, theta, torch.ones_like(theta))
    axis = cf / safe_theta
    half = safe_theta * (dt / 2)
    p = axis * torch.sin(half)
    p_w = torch.cos(half)
    q_x, q_y, q_z, q_w = q[0].clone(), q[1].clone(), q[2].clone(), q[3].clone()
    n = torch.stack((q_x * p_w + q_w * p[0] - q_z * p[1] + q_y * p[2],
                     q_y * p_w + q_z * p[0] + q_w * p[1] - q_x * p[2],
                     q_z * p_w - q_y * p[0] + q_x * p[1] + q_w * p[2],
                     q_w * p_w - q_x * p[0] - q_y * p[1] - q_z * p[2]), 0)
    n = n * ((3.0 - (n * n).sum(0)) / 2)
    q.copy_(torch.where(moving, n, q))
    bias_hat.copy_(torch.where(moving, bias_hat - ki * dt * omega_mes, bias_hat))
