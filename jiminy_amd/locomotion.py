"""Host side of the locomotion quantities block: from a `CompiledModel` and the frame names of a `blocks.FrameKinematics` to
the plan `jm_block_locomotion` interprets on the device.

Reference: python/gym_jiminy/common/gym_jiminy/common/quantities/locomotion.py -- `sanitize_foot_frame_names` (:31-84), the
grouping of the contact constraints by foot of `MultiFootNormalizedForceVertical.initialize` (:1400-1463) and the natural
frequency of `CapturePoint.initialize` (:1097-1112).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Sequence, Tuple, Union

import numpy as np

from . import _abi
from ._plan import fill_desc
from .frames import LOCAL, LOCAL_WORLD_ALIGNED, reference_frame
from .model import CompiledModel


def leaf_joints(model: CompiledModel) -> List[int]:
    """Joints no other joint has as parent (:45-48)."""
    return sorted(set(range(model.njoints)) - {int(p) for p in model.parents})


def sanitize_foot_frame_names(model: CompiledModel, frame_names: Union[Sequence[str], str] = "auto") -> List[str]:
    """≙ `sanitize_foot_frame_names` (:31-84).  'auto': the parent joint of every contact or force sensor on a leaf joint."""
    if not model.has_freeflyer:
        raise ValueError("Only legged robot with floating base are supported.")
    leaves = set(leaf_joints(model))
    # (every joint is a frame of its own name, as in the reference's model)
    leaf_frame_names = {name for name, fr in model.frames.items() if int(fr.parent_joint) in leaves} | {model.joint_names[j] for j in leaves}
    if isinstance(frame_names, str):
        if frame_names != "auto":
            raise ValueError("foot_frame_names must be 'auto' or a sequence of frame names")
        found = set()
        for sensor_type in ("ContactSensor", "ForceSensor"):
            for sensor in model.sensors.get(sensor_type, ()):
                if sensor["frame"] in leaf_frame_names:
                    found.add(model.joint_names[int(model.frames[sensor["frame"]].parent_joint)])
        frame_names = tuple(found)
    if not frame_names:
        raise ValueError("At least one frame must be specified.")
    if any(name not in leaf_frame_names for name in frame_names):
        raise ValueError("All frames must correspond to end-effectors.")
    return sorted(frame_names)


def group_contacts(model: CompiledModel, foot_frame_names: Sequence[str]) -> List[int]:
    """Foot index of every contact point of the model (-1: the contact belongs to no foot).  The contacts of one foot must
    be consecutive (:1440-1449)."""
    # (a name that is a joint's stands for the joint, whatever body frame shares it)
    foot_joints = [model.joint_names.index(name) if name in model.joint_names else int(model.frame(name).parent_joint)
                   for name in foot_frame_names]
    feet = [foot_joints.index(j) if j in foot_joints else -1 for j in (int(model.frame(c).parent_joint) for c in model.contacts)]
    for f in sorted(set(feet) - {-1}):
        first, last = feet.index(f), len(feet) - feet[::-1].index(f)
        if any(g != f for g in feet[first:last]):
            raise ValueError("Contact frames associated with identical parent body must be consecutive.")
    return feet


def neutral_placements(model: CompiledModel) -> Tuple[np.ndarray, np.ndarray]:
    """World rotation and position of every joint at the neutral configuration, where every joint motion is the identity."""
    R, p = np.zeros((model.njoints, 3, 3)), np.zeros((model.njoints, 3))
    R[0] = np.eye(3)
    for j in range(1, model.njoints):
        k = int(model.parents[j])
        R[j] = R[k] @ model.placement_R[j]
        p[j] = p[k] + R[k] @ model.placement_p[j]
    return R, p


def natural_frequency(model: CompiledModel) -> float:
    """≙ `CapturePoint.initialize` (:1097-1112): sqrt(g / (com_z - lowest contact frame z)) at the neutral configuration."""
    if not model.contacts:
        raise ValueError("the natural frequency of the capture point needs a model with contact frames")
    R, p = neutral_placements(model)
    mass = float(np.sum(model.mass[1:]))
    com_z = sum(float(model.mass[j]) * (p[j] + R[j] @ model.com[j])[2] for j in range(1, model.njoints)) / mass
    min_height = min((p[j] + R[j] @ fr.p)[2] for fr in map(model.frame, model.contacts) for j in (int(fr.parent_joint),))
    height = com_z - min_height
    if not height > 0.0:
        raise ValueError("the centre of mass of the neutral configuration is not above the lowest contact frame")
    return math.sqrt(abs(float(model.gravity[2])) / height)


@dataclass
class LocomotionPlan:
    foot_frame_names: List[str]
    contact_foot: List[int]
    omega: float
    arrays: Dict[str, Any] = field(default_factory=dict)

    @property
    def n_feet(self) -> int:
        return len(self.foot_frame_names)

    @property
    def n_contacts(self) -> int:
        return len(self.contact_foot)

    def desc(self) -> Tuple["_abi.LocomotionDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(*, body_mass, root_inertia, gravity: float, omega: float, contact_foot, contact_column, n_feet: int, n_frames: int,
              root_column: int, zmp_frame: int, dcm_frame: int) -> Tuple["_abi.LocomotionDesc", List[np.ndarray]]:
    """`jm_locomotion_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.LocomotionDesc()
    a, keep = fill_desc(d, dict(contact_foot=contact_foot, contact_column=contact_column),
                        dict(body_mass=body_mass, root_inertia=root_inertia))
    d.njoints, d.n_contacts, d.n_feet = len(a["body_mass"]), len(a["contact_foot"]), int(n_feet)
    d.gravity, d.omega = float(gravity), float(omega)
    d.n_frames, d.root_column, d.zmp_frame, d.dcm_frame = int(n_frames), int(root_column), int(zmp_frame), int(dcm_frame)
    return d, keep


def odometry_frame(mode: Union[int, str]) -> int:
    """LOCAL (the odometry frame) or LOCAL_WORLD_ALIGNED (:947-950, :1056-1059)."""
    m = reference_frame(mode)
    if m not in (LOCAL, LOCAL_WORLD_ALIGNED):
        raise ValueError("Reference frame must be either 'LOCAL' or 'LOCAL_WORLD_ALIGNED'.")
    return m


def build_plan(model: CompiledModel, frame_names: Sequence[str], *, foot_frame_names: Union[Sequence[str], str] = "auto",
               zmp_reference_frame: Union[int, str] = "LOCAL", dcm_reference_frame: Union[int, str] = "LOCAL") -> LocomotionPlan:
    """The plan of the locomotion quantities of `model`; `frame_names`: the frames of the frame kinematics block whose tensors
    the kernel reads, which must hold 'root_joint' and every contact frame."""
    feet = sanitize_foot_frame_names(model, foot_frame_names)
    if not model.contacts:
        raise ValueError("the locomotion quantities need a model with contact frames")
    frame_names = list(frame_names)
    missing = [n for n in ["root_joint"] + list(model.contacts) if n not in frame_names]
    if missing:
        raise ValueError(f"the frame kinematics block lacks the frames {missing}")
    contact_foot = group_contacts(model, feet)
    omega = natural_frequency(model)
    I = model.inertia[1]
    arrays = dict(body_mass=np.asarray(model.mass, dtype=np.float64),
                  root_inertia=np.array([I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]]),
                  gravity=abs(float(model.gravity[2])), omega=omega, contact_foot=contact_foot,
                  contact_column=[frame_names.index(c) for c in model.contacts], n_feet=len(feet), n_frames=len(frame_names),
                  root_column=frame_names.index("root_joint"), zmp_frame=odometry_frame(zmp_reference_frame),
                  dcm_frame=odometry_frame(dcm_reference_frame))
    return LocomotionPlan(foot_frame_names=feet, contact_foot=contact_foot, omega=omega, arrays=arrays)
