"""Host side of the tracking windows block: from the window horizons and the sizes of the source blocks to the plan
`jm_block_tracking` interprets on the device.

Reference: python/gym_jiminy/common/gym_jiminy/common -- the stack length of `DeltaBaseOdometryPosition.__init__` /
`DeltaBaseOdometryOrientation.__init__` (quantities/locomotion.py:1572-1573, :1666-1667) and of
`ShiftTrackingQuantityTermination.__init__` (compositions/generic.py:429-430), each with its assertion `horizon >= env.step_dt`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

from . import _abi

# launch modes of `jm_block_tracking`
RESTART, PUSH = 0, 1
# caps of csrc/jm_tracking.h
MAX_STACK, MAX_REL, MAX_MOTORS = 1024, 63, 256
# rows of the `scalars` tensor
SCALARS = ("drift_odom_position", "drift_odom_orientation", "reward_odom_pose", "shift_foot_positions", "shift_foot_orientations",
           "shift_motor_positions")


def stack_length(horizon: float, step_dt: float, what: str = "horizon") -> int:
    """≙ `max(int(np.ceil(horizon / env.step_dt)), 1) + 1` behind `assert horizon >= env.step_dt`, in float64."""
    if not (math.isfinite(step_dt) and step_dt > 0.0):
        raise ValueError("the tracking windows need the environment step: step_dt must be positive and finite")
    if not math.isfinite(horizon):
        raise ValueError(f"{what} must be finite")
    if not float(horizon) >= float(step_dt):
        raise ValueError(f"{what} must not be below step_dt (the reference asserts horizon >= env.step_dt)")
    max_stack = max(int(math.ceil(float(horizon) / float(step_dt))), 1) + 1
    if max_stack > MAX_STACK:
        raise ValueError(f"{what} / step_dt gives a window of {max_stack} steps: at most {MAX_STACK}")
    return max_stack


@dataclass
class TrackingPlan:
    max_stack_odom: int         # 0: the family is absent
    max_stack_foot: int
    max_stack_motor: int
    n_rel: int                  # F - 1, 0 without the foot family
    n_motors: int               # 0 without the motor family

    def desc(self) -> Tuple["_abi.TrackingDesc", List]:
        return make_desc(max_stack_odom=self.max_stack_odom, max_stack_foot=self.max_stack_foot,
                         max_stack_motor=self.max_stack_motor, n_rel=self.n_rel, n_motors=self.n_motors)


def make_desc(*, max_stack_odom: int, max_stack_foot: int, max_stack_motor: int, n_rel: int, n_motors: int
              ) -> Tuple["_abi.TrackingDesc", List]:
    """`jm_tracking_desc` from plain numbers (layout: include/jiminy_hip.h); the second value is empty, the description has no
    array to keep alive (the siblings' signature)."""
    d = _abi.TrackingDesc()
    d.max_stack_odom, d.max_stack_foot, d.max_stack_motor = int(max_stack_odom), int(max_stack_foot), int(max_stack_motor)
    d.n_rel, d.n_motors = int(n_rel), int(n_motors)
    return d, []


def build_plan(*, step_dt: float, odometry_horizon: Optional[float] = None, foot_horizon: Optional[float] = None,
               motor_horizon: Optional[float] = None, n_feet: Optional[int] = None, n_motors: Optional[int] = None) -> TrackingPlan:
    """The plan of the tracking windows: a horizon selects its family.  `n_feet` (F of the foot pose quantities) goes with
    `foot_horizon`, `n_motors` with `motor_horizon`."""
    if odometry_horizon is None and foot_horizon is None and motor_horizon is None:
        raise ValueError("the tracking windows need at least one of odometry_horizon, foot_horizon and motor_horizon")
    step_dt = float(step_dt)
    stack = lambda h, what: 0 if h is None else stack_length(float(h), step_dt, what)      # noqa: E731
    n_rel = 0
    if foot_horizon is not None:
        if n_feet is None:
            raise ValueError("foot_horizon needs the number of feet")
        if int(n_feet) < 2:
            raise ValueError("the relative foot poses of a single foot are empty: the foot windows need two feet or more")
        if int(n_feet) - 1 > MAX_REL:
            raise ValueError(f"the foot windows take at most {MAX_REL + 1} feet")
        n_rel = int(n_feet) - 1
    if motor_horizon is not None:
        if n_motors is None or int(n_motors) < 1:
            raise ValueError("motor_horizon needs a model with motors")
        if int(n_motors) > MAX_MOTORS:
            raise ValueError(f"the motor windows take at most {MAX_MOTORS} motors")
    return TrackingPlan(max_stack_odom=stack(odometry_horizon, "odometry_horizon"), max_stack_foot=stack(foot_horizon, "foot_horizon"),
                        max_stack_motor=stack(motor_horizon, "motor_horizon"), n_rel=n_rel,
                        n_motors=int(n_motors) if motor_horizon is not None else 0)
