"""Host side of the frame kinematics block: from a `CompiledModel` and a list of frame names to the plan
`jm_block_frame_kinematics` / `jm_block_frame_average` interpret on the device.

Reference: the quantities of python/gym_jiminy/common/gym_jiminy/common/quantities/generic.py that read `pinocchio_data.oMf`
and `getFrameVelocity` -- `FramePosition`, `FrameOrientation`, `FrameXYZQuat` (:298-950), `AverageFrameXYZQuat`,
`AverageFrameRollPitch`, `FrameSpatialAverageVelocity` (:1208-1534) -- and `BaseSpatialAverageVelocity` of
quantities/locomotion.py (:222-288), whose odometry frame is the third reference frame here.

The pose of a frame is a walk from the universe to the frame over the configuration: one segment per joint of the path,
each the placement of the joint on its parent followed by the motion of the joint read from `q` and `v`, and a trailing
constant segment with the placement of the frame on its parent joint.  A frame on the universe is that segment alone.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _abi
from ._plan import AXIS_KIND, SEG_FREEFLYER, SEG_PAXIS, SEG_PX, SEG_QUAT, SEG_UNBOUNDED, PlacedSegmentTable, fill_desc
from .model import (JT_FREEFLYER, JT_PU, JT_PX, JT_PY, JT_PZ, JT_RUBU, JT_RUBX, JT_RUBY, JT_RUBZ, JT_SPHERICAL,
                    CompiledModel)

# reference frames (≙ `pin.LOCAL`, `pin.LOCAL_WORLD_ALIGNED`; ODOMETRY: the step average only, locomotion.py:230-234)
LOCAL, LOCAL_WORLD_ALIGNED, ODOMETRY = 0, 1, 2
REFERENCE_FRAMES = {"LOCAL": LOCAL, "LOCAL_WORLD_ALIGNED": LOCAL_WORLD_ALIGNED, "ODOMETRY": ODOMETRY}
MAX_SEGS_PER_FRAME = 256


def reference_frame(mode: Union[int, str]) -> int:
    if isinstance(mode, str):
        if mode not in REFERENCE_FRAMES:
            raise ValueError(f"unknown reference frame '{mode}' (one of {sorted(REFERENCE_FRAMES)})")
        return REFERENCE_FRAMES[mode]
    if int(mode) not in (LOCAL, LOCAL_WORLD_ALIGNED, ODOMETRY):
        raise ValueError(f"unknown reference frame {mode}")
    return int(mode)


@dataclass
class FramePlan:
    frame_names: List[str]
    modes: List[int]
    depth: List[int]                             # segments per frame
    arrays: Dict[str, Any] = field(default_factory=dict)

    @property
    def n_frames(self) -> int:
        return len(self.frame_names)

    def desc(self) -> Tuple["_abi.FramesDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(*, nq: int, nv: int, njoints: int, frame_seg_start, frame_mode, seg_kind, seg_joint, seg_q_index, seg_v_index,
              seg_rot, seg_trans, seg_axis) -> Tuple["_abi.FramesDesc", List[np.ndarray]]:
    """`jm_frames_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.FramesDesc()
    a, keep = fill_desc(d, dict(frame_seg_start=frame_seg_start, frame_mode=frame_mode, seg_kind=seg_kind, seg_joint=seg_joint,
                                seg_q_index=seg_q_index, seg_v_index=seg_v_index),
                        dict(seg_rot=seg_rot, seg_trans=seg_trans, seg_axis=seg_axis))
    d.n_frames, d.nq, d.nv, d.njoints, d.n_seg = len(a["frame_mode"]), int(nq), int(nv), int(njoints), len(a["seg_kind"])
    return d, keep


def joint_segment(model: CompiledModel, j: int):
    """(kind, first q row, first v row, axis) of joint j as a segment of a walk (`PlacedSegmentTable.add_placed_frame`)."""
    t, iq, iv = int(model.jtypes[j]), int(model.idx_q[j]), int(model.idx_v[j])
    if t in AXIS_KIND:
        return AXIS_KIND[t], iq, iv, model.axes[j]
    if t in (JT_RUBX, JT_RUBY, JT_RUBZ, JT_RUBU):
        return SEG_UNBOUNDED, iq, iv, model.axes[j] if t == JT_RUBU else np.eye(3)[t - JT_RUBX]
    if t in (JT_PX, JT_PY, JT_PZ):
        return SEG_PX + (t - JT_PX), iq, iv, np.eye(3)[t - JT_PX]
    if t == JT_PU:
        return SEG_PAXIS, iq, iv, model.axes[j]
    if t == JT_SPHERICAL:
        return SEG_QUAT, iq, iv, np.zeros(3)
    if t == JT_FREEFLYER:
        return SEG_FREEFLYER, iq, iv, np.zeros(3)
    raise NotImplementedError(f"joint type {t} of joint '{model.joint_names[j]}'")


def build_plan(model: CompiledModel, frame_names: Sequence[str],
               reference_frames: Optional[Sequence[Union[int, str]]] = None) -> FramePlan:
    """The plan of the frame kinematics for the named frames, in the given order.  `reference_frames`: one of LOCAL,
    LOCAL_WORLD_ALIGNED, ODOMETRY per frame (default LOCAL)."""
    frame_names = list(frame_names)
    if not frame_names:
        raise ValueError("the frame kinematics need at least one frame")
    if reference_frames is None:
        reference_frames = [LOCAL] * len(frame_names)
    modes = [reference_frame(m) for m in reference_frames]
    if len(modes) != len(frame_names):
        raise ValueError(f"expected one reference frame per frame ({len(frame_names)}), got {len(modes)}")
    segs = PlacedSegmentTable()

    for name in frame_names:
        try:
            fr = model.frame(name)
        except LookupError:
            raise LookupError(f"frame '{name}' not found in model") from None
        segs.add_placed_frame(model, int(fr.parent_joint), fr.R, fr.p, lambda j: joint_segment(model, j))
    depth = list(np.diff(segs.frame_seg_start))
    if max(depth) > MAX_SEGS_PER_FRAME:
        raise NotImplementedError(f"a frame deeper than {MAX_SEGS_PER_FRAME} segments")
    arrays = dict(nq=int(model.nq), nv=int(model.nv), njoints=int(model.njoints), frame_seg_start=segs.frame_seg_start,
                  frame_mode=modes, seg_kind=segs.kind, seg_joint=segs.joint, seg_q_index=segs.index, seg_v_index=segs.v_index,
                  seg_rot=np.array(segs.rot), seg_trans=np.array(segs.trans), seg_axis=np.array(segs.axis))
    return FramePlan(frame_names=frame_names, modes=modes, depth=[int(n) for n in depth], arrays=arrays)
