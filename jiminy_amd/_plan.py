"""What the plan builders of the observer blocks and of the frame kinematics share (deformation.py, attitude.py, frames.py):
the segments of a frame and the marshalling of a plan description."""
from __future__ import annotations

import ctypes as C
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

from .model import JT_RU, JT_RX, JT_RY, JT_RZ, CompiledModel

# joint kinds of a plan segment (include/jiminy_hip.h: jm_deform_desc knows the first five, jm_attitude_desc all)
SEG_NONE, SEG_X, SEG_Y, SEG_Z, SEG_AXIS, SEG_UNBOUNDED, SEG_QUAT = range(7)
AXIS_KIND = {JT_RX: SEG_X, JT_RY: SEG_Y, JT_RZ: SEG_Z, JT_RU: SEG_AXIS}
# further kinds of jm_frames_desc, where SEG_QUAT is the spherical joint alone
SEG_FREEFLYER, SEG_PX, SEG_PY, SEG_PZ, SEG_PAXIS = range(7, 12)


class SegmentTable:
    """Frames as lists of segments, a segment being a constant rotation followed by the rotation of one joint."""

    def __init__(self) -> None:
        self.kind: List[int] = []
        self.index: List[int] = []
        self.rot: List[np.ndarray] = []
        self.axis: List[np.ndarray] = []
        self.ratio: List[float] = []
        self.frame_seg_start = [0]

    def _append(self, const: np.ndarray, kind: int, index: int, axis, ratio: float) -> None:
        self.kind.append(kind)
        self.index.append(index)
        self.rot.append(const)
        self.axis.append(np.asarray(axis, dtype=np.float64))
        self.ratio.append(ratio)

    def add_frame(self, model: CompiledModel, joint: int, R_frame, joint_segment: Callable[[int], Optional[tuple]]) -> int:
        """Walk from the root to the frame rigidly attached to `joint` with rotation `R_frame`; `joint_segment(j)` says
        what joint j contributes: (kind, index of what its rotation is read from, axis, ratio), or None (its placement
        joins the next constant rotation).  A trailing constant segment is emitted when it is not the identity, or when
        the frame would have no segment at all.  Returns the index of the frame in the table."""
        path, j = [], joint
        while j != 0:
            path.append(j)
            j = int(model.parents[j])
        const = np.eye(3)
        for j in reversed(path):
            const = const @ model.placement_R[j]
            seg = joint_segment(j)
            if seg is not None:
                self._append(const, *seg)
                const = np.eye(3)
        const = const @ np.asarray(R_frame, dtype=np.float64)
        if len(self.kind) == self.frame_seg_start[-1] or not np.array_equal(const, np.eye(3)):
            self._append(const, SEG_NONE, -1, np.zeros(3), 0.0)
        self.frame_seg_start.append(len(self.kind))
        return len(self.frame_seg_start) - 2


class PlacedSegmentTable(SegmentTable):
    """Frames as lists of segments with translations: a segment is a constant placement (rotation, translation) followed by
    the motion of one joint, of which the table also keeps the index and the first row of `v` (`index` is the first row of
    `q`).  Every joint of the path is a segment of its own, so that the placement of a segment is the placement of its joint
    alone; the trailing constant segment, always emitted, is the placement of the frame on its parent joint."""

    def __init__(self) -> None:
        super().__init__()
        self.trans: List[np.ndarray] = []
        self.joint: List[int] = []
        self.v_index: List[int] = []

    def add_placed_frame(self, model: CompiledModel, joint: int, R_frame, p_frame,
                         joint_segment: Callable[[int], tuple]) -> int:
        """Walk from the universe to the frame attached to `joint` with placement (`R_frame`, `p_frame`);
        `joint_segment(j)` gives (kind, first q row, first v row, axis) of joint j.  Returns the index of the frame."""
        path, j = [], joint
        while j != 0:
            path.append(j)
            j = int(model.parents[j])
        for j in reversed(path):
            kind, iq, iv, axis = joint_segment(j)
            self._append(np.asarray(model.placement_R[j], dtype=np.float64), kind, iq, axis, 0.0)
            self.trans.append(np.asarray(model.placement_p[j], dtype=np.float64))
            self.joint.append(j)
            self.v_index.append(iv)
        self._append(np.asarray(R_frame, dtype=np.float64), SEG_NONE, -1, np.zeros(3), 0.0)
        self.trans.append(np.asarray(p_frame, dtype=np.float64))
        self.joint.append(-1)
        self.v_index.append(-1)
        self.frame_seg_start.append(len(self.kind))
        return len(self.frame_seg_start) - 2


def fill_desc(desc, ints: Dict[str, Any], dbls: Dict[str, Any]) -> Tuple[Dict[str, np.ndarray], List[np.ndarray]]:
    """Point the fields of the ctypes description `desc` at flat int32 / float64 copies of the given arrays.  Returns
    the copies by name, and as the list that keeps them alive."""
    flat = {k: np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.int32) for k, v in ints.items()}
    flat.update({k: np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.float64) for k, v in dbls.items()})
    for k, a in flat.items():
        setattr(desc, k, a.ctypes.data_as(C.POINTER(C.c_int32 if k in ints else C.c_double)))
    return flat, list(flat.values())
