"""Host side of the foot pose quantities block: from a `CompiledModel` and the frame names of a `blocks.FrameKinematics` to the
plan `jm_block_foot_poses` interprets on the device.

Reference: python/gym_jiminy/common/gym_jiminy/common/quantities/locomotion.py -- `sanitize_foot_frame_names` (:31-84), whose
sorted names are the order of the feet in `MultiFootMeanXYZQuat` (:416-478) and `MultiFootRelativeXYZQuat` (:702-810): the
last of them is the foot the relative poses drop.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Sequence, Tuple, Union

import numpy as np

from . import _abi
from ._plan import fill_desc
from .locomotion import sanitize_foot_frame_names
from .model import CompiledModel

# cap of csrc/jm_footposes.h
MAX_FEET = 64


@dataclass
class FootPosesPlan:
    foot_frame_names: List[str]
    arrays: Dict[str, Any] = field(default_factory=dict)

    @property
    def n_feet(self) -> int:
        return len(self.foot_frame_names)

    @property
    def n_frames(self) -> int:
        return int(self.arrays["n_frames"])

    def desc(self) -> Tuple["_abi.FootPosesDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(*, foot_column, n_frames: int) -> Tuple["_abi.FootPosesDesc", List[np.ndarray]]:
    """`jm_footposes_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.FootPosesDesc()
    a, keep = fill_desc(d, dict(foot_column=foot_column), {})
    d.n_feet, d.n_frames = len(a["foot_column"]), int(n_frames)
    return d, keep


def build_plan(model: CompiledModel, frame_names: Sequence[str], foot_frame_names: Union[Sequence[str], str] = "auto") -> FootPosesPlan:
    """The plan of the foot pose quantities of `model`; `frame_names`: the frames of the frame kinematics block whose `pose`
    the kernel reads, which must hold every foot frame."""
    feet = sanitize_foot_frame_names(model, foot_frame_names)
    if len(feet) > MAX_FEET:
        raise ValueError(f"at most {MAX_FEET} feet are supported, got {len(feet)}")
    frame_names = list(frame_names)
    missing = [n for n in feet if n not in frame_names]
    if missing:
        raise ValueError(f"the frame kinematics block lacks the foot frames {missing}")
    arrays = dict(foot_column=[frame_names.index(n) for n in feet], n_frames=len(frame_names))
    return FootPosesPlan(foot_frame_names=feet, arrays=arrays)
