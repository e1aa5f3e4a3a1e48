"""Host side of the centroidal state block: from a `CompiledModel` to the plan `jm_block_centroidal_state` interprets on the
device.

Reference: `pin.computeCentroidalMomentumTimeVariation` on the state of a trajectory (python/jiminy_py/src/jiminy_py/
dynamics.py:496-499, reached from `StateQuantity.refresh`, python/gym_jiminy/common/gym_jiminy/common/bases/quantities.py:
1494-1518).  The plan is that of the nominal model: the reference evaluates a trajectory on the trajectory's own robot.

A body is a walk from the universe to its joint frame in the segment tables of the frame kinematics (`frames.py`), with its
mass, its centre of mass and its inertia about it.  Bodies without mass and inertia are left out.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Tuple

import numpy as np

from . import _abi
from ._plan import PlacedSegmentTable, fill_desc
from .frames import MAX_SEGS_PER_FRAME, joint_segment
from .model import CompiledModel

ROWS = 15       # com (3), hg (6), dhg (6): the rows of the engine's `centroidal` field


@dataclass
class CentroidalPlan:
    joints: List[int]                            # the joint of every body of the plan
    depth: List[int]                             # segments per body
    mass: float
    arrays: Dict[str, Any] = field(default_factory=dict)

    @property
    def n_bodies(self) -> int:
        return len(self.joints)

    def desc(self) -> Tuple["_abi.CentroidalDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(*, nq: int, nv: int, njoints: int, body_seg_start, seg_kind, seg_joint, seg_q_index, seg_v_index, seg_rot, seg_trans,
              seg_axis, body_mass, body_com, body_inertia) -> Tuple["_abi.CentroidalDesc", List[np.ndarray]]:
    """`jm_centroidal_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.CentroidalDesc()
    a, keep = fill_desc(d, dict(body_seg_start=body_seg_start, seg_kind=seg_kind, seg_joint=seg_joint, seg_q_index=seg_q_index,
                                seg_v_index=seg_v_index),
                        dict(seg_rot=seg_rot, seg_trans=seg_trans, seg_axis=seg_axis, body_mass=body_mass, body_com=body_com,
                             body_inertia=body_inertia))
    d.n_bodies, d.nq, d.nv, d.njoints, d.n_seg = len(a["body_mass"]), int(nq), int(nv), int(njoints), len(a["seg_kind"])
    return d, keep


def build_plan(model: CompiledModel) -> CentroidalPlan:
    """The plan of the centroidal quantities of the nominal `model`."""
    joints = [j for j in range(1, model.njoints) if float(model.mass[j]) != 0.0 or np.any(model.inertia[j] != 0.0)]
    if not joints or not float(np.sum(model.mass[joints])) > 0.0:
        raise ValueError("the centroidal quantities need a model with mass")
    segs = PlacedSegmentTable()
    for j in joints:
        segs.add_placed_frame(model, j, np.eye(3), np.zeros(3), lambda i: joint_segment(model, i))
    depth = [int(n) for n in np.diff(segs.frame_seg_start)]
    if max(depth) > MAX_SEGS_PER_FRAME:
        raise NotImplementedError(f"a body deeper than {MAX_SEGS_PER_FRAME} segments")
    I = np.asarray(model.inertia, dtype=np.float64)[joints]
    arrays = dict(nq=int(model.nq), nv=int(model.nv), njoints=int(model.njoints), body_seg_start=segs.frame_seg_start,
                  seg_kind=segs.kind, seg_joint=segs.joint, seg_q_index=segs.index, seg_v_index=segs.v_index,
                  seg_rot=np.array(segs.rot), seg_trans=np.array(segs.trans), seg_axis=np.array(segs.axis),
                  body_mass=np.asarray(model.mass, dtype=np.float64)[joints], body_com=np.asarray(model.com, dtype=np.float64)[joints],
                  body_inertia=np.stack([I[:, 0, 0], I[:, 0, 1], I[:, 0, 2], I[:, 1, 1], I[:, 1, 2], I[:, 2, 2]], axis=1))
    return CentroidalPlan(joints=joints, depth=depth, mass=float(np.sum(model.mass[joints])), arrays=arrays)
