"""Host side of the actuated-joint quantities block: from a `CompiledModel` to the plan `jm_block_actuation` interprets on the
device.

Reference: python/gym_jiminy/common/gym_jiminy/common/quantities/generic.py -- `MultiActuatedJointKinematic.initialize`
(:1613-1673: the rows and the mechanical reduction of every motor, in motor order), `EnergyGenerationMode` (:1694-1719) and the
stack length of `AverageMechanicalPowerConsumption.__init__` (:1865) -- and compositions/generic.py --
`_MultiActuatedJointBoundDistance.initialize` (:486-498: the position bounds at the motors' rows).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np

from . import _abi
from ._plan import fill_desc
from .model import JT_RUBU, JT_RUBX, JT_RUBY, JT_RUBZ, CompiledModel

# `EnergyGenerationMode` (quantities/generic.py:1694-1719)
GENERATOR_MODES = {"CHARGE": 0, "LOST_EACH": 1, "LOST_GLOBAL": 2, "PENALIZE": 3}
# launch modes of `jm_block_actuation`
RESTART, PUSH = 0, 1
# caps of csrc/jm_actuation.h
MAX_MOTORS, MAX_STACK = 256, 1024


def energy_generation_mode(mode: Union[int, str]) -> int:
    """`EnergyGenerationMode` by name or by value."""
    if isinstance(mode, str):
        if mode.upper() not in GENERATOR_MODES:
            raise ValueError(f"generator_mode must be one of {', '.join(GENERATOR_MODES)}")
        return GENERATOR_MODES[mode.upper()]
    if int(mode) not in GENERATOR_MODES.values():
        raise ValueError(f"generator_mode must be one of {', '.join(GENERATOR_MODES)} (0 .. 3)")
    return int(mode)


def stack_length(power_horizon: float, step_dt: float) -> int:
    """≙ `max(int(np.ceil(horizon / env.step_dt)), 1) + 1` (quantities/generic.py:1865), in float64."""
    if not (math.isfinite(power_horizon) and power_horizon > 0.0):
        raise ValueError("power_horizon must be positive and finite")
    if not (math.isfinite(step_dt) and step_dt > 0.0):
        raise ValueError("power_horizon needs the environment step: step_dt must be positive and finite")
    return max(int(math.ceil(float(power_horizon) / float(step_dt))), 1) + 1


@dataclass
class ActuationPlan:
    motor_names: List[str]
    generator_mode: int
    max_stack: int
    has_horizon: bool
    arrays: Dict[str, Any] = field(default_factory=dict)

    @property
    def n_motors(self) -> int:
        return len(self.motor_names)

    def desc(self) -> Tuple["_abi.ActuationDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(*, idx_q, idx_v, reduction, position_low, position_high, nq: int, nv: int, generator_mode: int,
              max_stack: int) -> Tuple["_abi.ActuationDesc", List[np.ndarray]]:
    """`jm_actuation_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.ActuationDesc()
    a, keep = fill_desc(d, dict(idx_q=idx_q, idx_v=idx_v),
                        dict(reduction=reduction, position_low=position_low, position_high=position_high))
    d.n_motors, d.nq, d.nv = len(a["idx_q"]), int(nq), int(nv)
    d.generator_mode, d.max_stack = int(generator_mode), int(max_stack)
    return d, keep


def build_plan(model: CompiledModel, *, generator_mode: Union[int, str] = "CHARGE", power_horizon: Optional[float] = None,
               step_dt: Optional[float] = None) -> ActuationPlan:
    """The plan of the actuated-joint quantities of `model`: its motors in `model.motors` order.  Without a horizon the plan
    carries the smallest window (`max_stack = 2`) and `has_horizon` is False."""
    mode = energy_generation_mode(generator_mode)
    if not model.motors:
        raise ValueError("the actuated-joint quantities need a model with motors")
    if len(model.motors) > MAX_MOTORS:
        raise ValueError(f"the actuated-joint quantities take at most {MAX_MOTORS} motors")
    for m in model.motors:
        if int(model.jtypes[m.joint]) in (JT_RUBX, JT_RUBY, JT_RUBZ, JT_RUBU):
            raise ValueError("Revolute unbounded joints are not supported for now.")       # (quantities/generic.py:1634-1636)
    max_stack = 2
    if power_horizon is not None:
        if step_dt is None:
            raise ValueError("power_horizon needs the environment step: give step_dt")
        max_stack = stack_length(float(power_horizon), float(step_dt))
        if max_stack > MAX_STACK:
            raise ValueError(f"power_horizon / step_dt gives a window of {max_stack} steps: at most {MAX_STACK}")
    idx_q = [int(m.idx_q) for m in model.motors]
    arrays = dict(idx_q=idx_q, idx_v=[int(m.idx_v) for m in model.motors], reduction=[float(m.reduction) for m in model.motors],
                  position_low=np.asarray(model.position_lower, dtype=np.float64)[idx_q],
                  position_high=np.asarray(model.position_upper, dtype=np.float64)[idx_q],
                  nq=model.nq, nv=model.nv, generator_mode=mode, max_stack=max_stack)
    return ActuationPlan(motor_names=[m.name for m in model.motors], generator_mode=mode, max_stack=max_stack,
                         has_horizon=power_horizon is not None, arrays=arrays)
