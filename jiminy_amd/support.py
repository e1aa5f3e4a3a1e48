"""Host side of the projected support polygon block: from a `CompiledModel` and the frame names of a `blocks.FrameKinematics` to
the plan `jm_block_support_polygon` interprets on the device.

Reference: python/gym_jiminy/toolbox/gym_jiminy/toolbox/quantities/locomotion.py -- `ProjectedSupportPolygon.initialize`
(:83-144): every contact frame of the robot is a candidate point, in the order of `robot.contact_frame_names`.  The
reference then drops, once, the points that are not vertices of the 3D convex hull of their body (scipy); that pruning does
not change the polygon and is not built: the plan lists every contact point, and `vertex_index` counts in the model's
contact order.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Sequence, Tuple, Union

import numpy as np

from . import _abi
from ._plan import fill_desc
from .locomotion import odometry_frame
from .model import CompiledModel

# cap of csrc/jm_support.h
MAX_POINTS = 16
SCALARS = ("stability_margin", "reward_robustness")


@dataclass
class SupportPlan:
    contact_names: List[str]
    arrays: Dict[str, Any] = field(default_factory=dict)

    @property
    def n_points(self) -> int:
        return len(self.contact_names)

    @property
    def n_frames(self) -> int:
        return int(self.arrays["n_frames"])

    @property
    def reference_frame(self) -> int:
        return int(self.arrays["reference_frame"])

    def desc(self) -> Tuple["_abi.SupportDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(*, point_column, n_frames: int, reference_frame: int) -> Tuple["_abi.SupportDesc", List[np.ndarray]]:
    """`jm_support_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.SupportDesc()
    a, keep = fill_desc(d, dict(point_column=point_column), {})
    d.n_points, d.n_frames, d.reference_frame = len(a["point_column"]), int(n_frames), int(reference_frame)
    return d, keep


def check_model(model: CompiledModel) -> None:
    """The refusals of `ProjectedSupportPolygon` (:83-95; a model here has no collision bodies) and the cap of the kernel."""
    if not model.has_freeflyer:
        raise RuntimeError("Only legged robot with floating base are supported: the model has no free-flyer.")
    if not model.contacts:
        raise RuntimeError("Only robots having at least one contact are supported.")
    if len(model.contacts) > MAX_POINTS:
        raise NotImplementedError(f"at most {MAX_POINTS} contact points are supported, got {len(model.contacts)} (the "
                                  "reference's pruning by the 3D hull of each body is not built)")


def build_plan(model: CompiledModel, frame_names: Sequence[str], reference_frame: Union[int, str] = "LOCAL") -> SupportPlan:
    """The plan of the projected support polygon of `model`; `frame_names`: the frames of the frame kinematics block whose
    `pose` the kernel reads, which must hold every contact frame."""
    check_model(model)
    frame = odometry_frame(reference_frame)
    frame_names = list(frame_names)
    missing = [n for n in model.contacts if n not in frame_names]
    if missing:
        raise ValueError(f"the frame kinematics block lacks the contact frames {missing}")
    arrays = dict(point_column=[frame_names.index(c) for c in model.contacts], n_frames=len(frame_names), reference_frame=frame)
    return SupportPlan(contact_names=list(model.contacts), arrays=arrays)
