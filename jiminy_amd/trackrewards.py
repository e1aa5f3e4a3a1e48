"""Host side of the tracking rewards block: the plan `jm_block_tracking_rewards` interprets on the device.

Reference: the `TrackingQuantityReward` family (python/gym_jiminy/common/gym_jiminy/common/compositions/generic.py:64-150,
compositions/locomotion.py:33-143) -- a quantity in `QuantityEvalMode.TRUE` against the same quantity in
`QuantityEvalMode.REFERENCE`.  The plan names the columns of 'root_joint' and of the contact frames (`BaseRelativeHeight`,
quantities/locomotion.py:130-138: the contact frames of the robot) in the tensors of the two frame kinematics blocks.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from ._plan import fill_desc
from .model import CompiledModel

TERMS = ("base_height", "odometry_velocity", "capture_point", "joint_positions")     # the rows of `rewards`
FIXED_ROWS = 6      # height (1), odometry velocity (3), capture point (2); the joint positions follow


@dataclass
class TrackRewardsPlan:
    n_motors: int
    arrays: Dict[str, Any] = field(default_factory=dict)

    @property
    def rows(self) -> int:
        return FIXED_ROWS + self.n_motors

    def desc(self) -> Tuple["_abi.TrackRewardsDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(*, n_motors: int, n_frames: int, root_column: int, contact_column, n_frames_reference: int, root_column_reference: int,
              contact_column_reference) -> Tuple["_abi.TrackRewardsDesc", List[np.ndarray]]:
    """`jm_trackrewards_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.TrackRewardsDesc()
    a, keep = fill_desc(d, dict(contact_column=contact_column, contact_column_reference=contact_column_reference), {})
    if len(a["contact_column"]) != len(a["contact_column_reference"]):
        raise ValueError("the two sides must name the same contact frames")
    d.n_contacts, d.n_motors = len(a["contact_column"]), int(n_motors)
    d.n_frames, d.root_column = int(n_frames), int(root_column)
    d.n_frames_reference, d.root_column_reference = int(n_frames_reference), int(root_column_reference)
    return d, keep


def build_plan(model: CompiledModel, frame_names: Optional[Sequence[str]], reference_frame_names: Optional[Sequence[str]],
               n_motors: int) -> TrackRewardsPlan:
    """The plan for the frames of the true and of the reference frame kinematics block (None: no such block; the terms that
    read one are then skipped)."""
    contacts = list(model.contacts)

    def side(names):
        if names is None:
            return 0, 0, [0] * len(contacts)
        names = list(names)
        missing = [n for n in ["root_joint"] + contacts if n not in names]
        if missing:
            raise ValueError(f"the frame kinematics block lacks the frames {missing}")
        return len(names), names.index("root_joint"), [names.index(c) for c in contacts]
    K, root, col = side(frame_names)
    Kr, root_r, col_r = side(reference_frame_names)
    arrays = dict(n_motors=int(n_motors), n_frames=K, root_column=root, contact_column=col, n_frames_reference=Kr,
                  root_column_reference=root_r, contact_column_reference=col_r)
    return TrackRewardsPlan(n_motors=int(n_motors), arrays=arrays)
